"""CPU: the cases of tests/rnn_case.py are what tests/test_gpu_rnn.py takes them for -- the tables cover the
dispatch's branches and say which path each case takes, every float32 floor makes a tight bar, another legitimate
float32 summation order keeps a factor 4 from that bar, and the checker rejects planted faults."""
import numpy as np
import pytest

import rnn_case as rc

ALL = rc.GRU_CASES + rc.LSTM_CASES
IDS = [f"{c.cell}-{rc.case_id(c)}" for c in ALL]


# --------------------------------------------------------------------------- the support rules, restated
# (csrc/gru_persist.hip gru_persist_supported / gru_persist_fused_xproj, csrc/lstm_persist.hip
# lstm_persist_supported, csrc/handoff.h chain_grid; a change to a rule in C++ has to be mirrored here knowingly)

def chain_grid(nchains, nmem):
    return 8 * nmem * ((nchains + 7) // 8)


def gru_persist_supported(nd, B, H):
    if H not in (64, 128, 256, 512):
        return False
    MT = (B + 15) // 16
    return (2 * H // 16) * ((nd * MT + 7) // 8) <= 32  # one workgroup per CU, 32 CUs per XCD


def gru_persist_fused_xproj(nd, B, H, Kx):
    if B > 64 or Kx % 32 != 0 or H % 64 != 0:
        return False
    nchains, nmem = nd * ((B + 15) // 16), 2 * H // 16
    return chain_grid(nchains, nmem) - nchains * nmem >= 32


def lstm_persist_supported(nd, B, H, peep):
    if peep or H not in (64, 128, 256):
        return False
    nchains, nmem = nd * ((B + 15) // 16), H // 16
    return nmem * ((nchains + 7) // 8) <= 32


def test_expected_paths_follow_the_support_rules():
    for c in rc.GRU_CASES:
        nd = rc.ndir(c)
        p = gru_persist_supported(nd, c.B, c.H)
        # the layer's x has ldx = D, a multiple of 4 whenever D % 32 == 0, in a 16-byte aligned allocation
        f = p and gru_persist_fused_xproj(nd, c.B, c.H, c.D)
        assert (c.path, c.fused) == (int(p), int(f)), rc.case_id(c)
    for c in rc.LSTM_CASES:
        assert c.path == int(lstm_persist_supported(rc.ndir(c), c.B, c.H, c.peep)), rc.case_id(c)
        assert c.fused is None


def test_tables_cover_what_they_are_for():
    ids = [(c.cell, rc.case_id(c)) for c in ALL]
    assert len(set(ids)) == len(ids)
    assert all(c.L <= 12 for c in ALL)
    for cell, cases, widths in (("gru", rc.GRU_CASES, (64, 128, 256)), ("lstm", rc.LSTM_CASES, (64, 128, 256))):
        pers = [c for c in cases if c.path == 1]
        for H in widths:
            assert any(c.H == H for c in pers), (cell, H)
            assert sum(c.ab for c in pers if c.H == H) == 1, (cell, H)  # one per-step arm per width
        assert all(c.path == 1 for c in cases if c.ab)
        # both chain rounds, and the fallback past the last supported batch
        assert any(rc.nchains(c) <= 8 for c in pers) and any(8 < rc.nchains(c) <= 16 for c in pers), cell
        assert any(rc.nchains(c) == 16 for c in pers), cell
        assert any(c.path == 0 and c.H == 256 and rc.nchains(c) == 18 for c in cases), cell
        # a uni reverse ragged case on each path, and a saturated leg on each path
        for path in (0, 1):
            assert any(c.dirn == "rev" and c.lengths == "ragged" and c.path == path for c in cases), (cell, path)
            assert any(c.data == "saturated" and c.path == path for c in cases), (cell, path)
    g = rc.GRU_CASES
    # H = 512 never fits an XCD: one round and two, uni and bi, and a saturated leg all take the per-step launches
    assert {4, 5, 8, 10} <= {rc.nchains(c) for c in g if c.H == 512} and all(c.path == 0 for c in g if c.H == 512)
    assert any(c.H == 512 and c.data == "saturated" for c in g)
    # the last supported and the first unsupported chain count of each persistent width the tables reach
    assert {(256, 8, 1), (256, 10, 0), (128, 16, 1), (128, 18, 0)} <= {(c.H, rc.nchains(c), c.path) for c in g}
    for H in (64, 128, 256):
        for fused in (0, 1):
            assert any(c.H == H and c.path == 1 and c.fused == fused for c in g), (H, fused)
    # short sequences on the persistent GRU: below, at and just past the 4-slot ring
    assert {1, 2, 3, 4, 5} <= {c.L for c in g if c.path == 1}
    # per-step widths above 64, and the width the persistent LSTM's dispatch used to let through
    assert {16, 48, 192, 320} <= {c.H for c in g if c.path == 0}
    lc = rc.LSTM_CASES
    assert any(c.H == 192 and not c.peep and c.path == 0 for c in lc)
    assert any(c.H == 192 and c.peep for c in lc) and any(c.H == 320 for c in lc)
    assert {(64, True), (256, True), (16, True), (16, False)} <= {(c.H, c.peep) for c in lc if c.path == 0}


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_case_builds_and_its_lengths_keep_the_ragged_rule(c):
    for leg in (0, 1):
        d = rc.build(c, leg)
        assert d.x.dtype == d.dy.dtype == np.float32
        assert d.x.shape == (c.B, c.L, c.D) and d.dy.shape == (c.B, c.L, rc.ndir(c) * c.H)
        assert len(d.W) == rc.ndir(c) and all(v.dtype == np.float32 for w in d.W for v in w.values())
        if leg == 0:
            assert (d.lens is not None) == (c.lengths == "ragged")
        else:  # the relaunch: other data, other lengths, the weights halved
            d0 = rc.build(c, 0)
            assert not np.array_equal(d.x, d0.x) and not np.array_equal(d.dy, d0.dy)
            assert all(np.array_equal(v, d0.W[i][k] * np.float32(0.5)) for i, w in enumerate(d.W) for k, v in w.items())
            assert (d.lens is not None) == (c.L >= 2)
            if d0.lens is not None and c.B >= 5 and c.L >= 2:
                assert not np.array_equal(d.lens, d0.lens)
        if d.lens is None:
            continue
        lens = d.lens
        assert lens.shape == (c.B,) and lens.min() >= 1 and lens.max() <= c.L
        assert lens[0] == c.L and lens[-1] == 1
        if c.B >= 4 and c.L >= 5:
            assert 4 in lens and 5 in lens
        if c.B > 16 and c.L >= 2:
            tiles = [lens[i:i + 16] for i in range(0, c.B, 16)]
            assert any((t < c.L).all() for t in tiles)
        # padding frames hold finite non-zero data: a kernel that reads them is caught
        pad = rc.reference(c, leg).pad
        assert np.array_equal(pad, np.arange(c.L)[None, :] >= lens[:, None])
        assert (d.x[pad] != 0).all()


@pytest.mark.parametrize("c", [c for c in ALL if c.data == "saturated"],
                         ids=[i for c, i in zip(ALL, IDS) if c.data == "saturated"])
def test_saturated_legs_saturate(c):
    r = rc.reference(c)
    assert r.sat_fraction >= 0.2, r.sat_fraction  # of z, r (i, f, o): below 1e-6 or above 1 - 1e-6
    assert r.preact_max > 88.0, r.preact_max      # where float32 expf overflows
    assert all(np.isfinite(v).all() for v in r.tensors.values())


def test_plain_legs_do_not_saturate():
    for c in ALL:
        if c.data == "plain":
            assert c.xscale == 1.0 and rc.reference(c).sat_fraction == 0.0, rc.case_id(c)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_floor_is_usable_and_factor_16_has_its_margin(c):
    """floor <= 1e-5 max|ref| for every tensor of both launches, so the bar min(16 floor, 1e-4 max|ref|) is its
    16 x floor arm or within a factor 1.6 of it; and the float32 restatement with every product summed in K-chunks
    of 16 stays within 4 floors of float64, which leaves a factor 4 between another correct fp32 order and the
    bar."""
    for leg in (0, 1):
        r64, r32 = rc.reference(c, leg), rc.reference(c, leg, np.float32)
        rch = rc.reference(c, leg, np.float32, True) if leg == 0 else None
        for k, v in r64.tensors.items():
            assert r32.tensors[k].dtype == np.float32 and v.dtype == np.float64
            scale = np.abs(v).max()
            assert scale > 0, (leg, k)
            floor = np.abs(r32.tensors[k] - v).max()
            assert floor <= 1e-5 * scale, (leg, k, floor, scale)
            if floor == 0:  # only a gradient whose every term is exactly 0 (h = 0 at the only step): the prefill
                assert c.L == 1 and (v == rc.PREFILL).all(), (leg, k)
            if rch is not None:
                assert rch.tensors[k].dtype == np.float32
                other = np.abs(rch.tensors[k] - v).max()
                assert other <= 4 * floor, (k, other, floor)
        if rch is not None:  # the chunked products do change the rounding: it is another order, not the same one
            assert any(not np.array_equal(rch.tensors[k], r32.tensors[k]) for k in r64.tensors)


def test_chunked_products_are_chunked():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((5, 70)).astype(np.float32)
    b = rng.standard_normal((70, 3)).astype(np.float32)
    want = a[:, :16] @ b[:16]
    for k in range(16, 70, 16):
        want = want + a[:, k:k + 16] @ b[k:k + 16]
    got = a.view(rc.ChunkedK) @ b
    assert isinstance(got, rc.ChunkedK) and got.dtype == np.float32
    assert np.array_equal(np.asarray(got), want)
    assert isinstance(np.concatenate([a, a.view(rc.ChunkedK)], axis=1), rc.ChunkedK)
    acc = np.zeros((5, 3), np.float32)
    acc += 0.5 * (a.view(rc.ChunkedK) @ b)
    assert type(acc) is np.ndarray and np.array_equal(acc, np.float32(0.5) * want)


def _got(c):
    return {k: v.copy() for k, v in rc.reference(c).tensors.items()}


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_checker_passes_the_references(c, capsys):
    """The float64 reference and both float32 restatements pass; the printed line names every figure."""
    rc.check_all(_got(c), c)
    out = capsys.readouterr().out
    assert out.count("fp32 restatement") == len(rc.reference(c).tensors) and "bar" in out
    ratios = rc.check_all(rc.reference(c, 0, np.float32).tensors, c)
    assert max(ratios.values()) == 1.0
    rc.check_all(rc.reference(c, 0, np.float32, True).tensors, c)


@pytest.mark.parametrize("fault", rc.FAULTS)
def test_checker_catches_planted_fault(fault):
    applies = [c for c in ALL if rc.fault_applies(c, fault)]
    assert len(applies) >= 8, (fault, len(applies))
    assert {"gru", "lstm"} == {c.cell for c in applies}
    for c in applies:
        bad = rc.reference(c, 0, np.float64, False, fault).tensors
        with pytest.raises(AssertionError):
            rc.check_all({k: v.copy() for k, v in bad.items()}, c)
        # and it is that fault's tensor that fails, not another one
        good = _got(c)
        changed = [k for k in good if not np.array_equal(good[k], bad[k])]
        assert changed, (fault, rc.case_id(c))
        for k in good:
            if k not in changed:
                r = rc.reference(c)
                rc.check(good[k], r.tensors[k], rc.reference(c, 0, np.float32).tensors[k], k)


def test_checker_zero_reference_and_shapes():
    z = np.zeros((2, 3))
    assert rc.check(np.full((2, 3), 1e-8), z, z, "zero") == 0.0
    with pytest.raises(AssertionError):
        rc.check(np.full((2, 3), 2e-7), z, z, "zero")
    with pytest.raises(AssertionError):
        rc.check(np.zeros((3, 2)), z, z, "shape")
    one = np.ones((2, 3))
    with pytest.raises(AssertionError):
        rc.check(np.full((2, 3), np.nan), one, one.astype(np.float32), "nan")
    c = rc.GRU_CASES[1]
    got = _got(c)
    got.pop("dx")
    with pytest.raises(AssertionError):
        rc.check_all(got, c)
