"""The attention-decoder cases of tests/dec_case.py are what tests/test_gpu_dec.py takes them for (no GPU): the
expected route columns follow the dispatch rules and cover every route, chain class and feature pair; the peaked
data meets its three conditions and no case has more than a few decisions inside the margins; the float32 floor of
every tensor is small enough to make min(16 x floor, 1e-4 max|ref|) the tight bar; another float32 summation order
keeps a factor 4 from it; and the checker rejects every planted fault on every case it applies to."""
import numpy as np
import pytest

import dec_case as dc

IDS = [dc.case_id(c) for c in dc.CASES]
LEGS = range(dc.NLEGS - 1)  # leg 3 is leg 0 again


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("c", dc.CASES, ids=IDS)
def test_expected_route_follows_the_dispatch_rules(c):
    path, plan, fold = dc.route(c)
    assert (path, plan, fold) == (c.path, c.plan, c.fold), (path, plan, fold)
    if c.persist_res is not None:  # 1: the resident candidate's shape; 0: chunks past the 128 workgroups of a tile
        assert c.path == dc.PERSIST and c.persist_res == int(16 * -(-c.L // 16) <= 128)
    for leg in (1, 2):  # the other legs stay on the case's route
        assert dc.route(c, *dc.leg_shape(c, leg))[0] == c.path, leg


def test_table_covers_every_route_and_feature_pair():
    def some(f):
        return any(f(c) for c in dc.CASES)

    for path in (dc.STEPS, dc.PERSIST, dc.XCD, dc.XCD_LSTM):
        assert some(lambda c: c.path == path), path
        assert some(lambda c: c.path == path and c.data == "peaked"), path
        assert some(lambda c: c.path == path and c.dropout > 0), path
    for path in (dc.XCD, dc.XCD_LSTM):  # U classes 1, 2..4; > 4 on XCD only (XCD_LSTM declines it)
        assert some(lambda c: c.path == path and c.plan[0] == 1)
        assert some(lambda c: c.path == path and 2 <= c.plan[0] <= 4)
        assert some(lambda c: c.path == path and c.lengths == "ragged")
    assert some(lambda c: c.path == dc.XCD and c.plan[0] > 4)
    assert {c.plan[4] for c in dc.CASES if c.path == dc.XCD} == {0, 1, 2}
    assert some(lambda c: c.path == dc.XCD and c.plan[4] == 1 and c.stream is None)  # naturally streamed
    assert some(lambda c: c.path == dc.XCD and (c.L - 1) % c.plan[2] == 0)  # a last chunk of one frame
    assert {c.persist_res for c in dc.CASES if c.path == dc.PERSIST} >= {0, 1}
    steps = [c for c in dc.CASES if c.path == dc.STEPS]
    assert {c.kW for c in steps if c.nF and c.cell == "gru"} >= {1, 4, 5, 8}
    assert {(c.cell, c.nF > 0) for c in steps} == {("gru", False), ("gru", True), ("lstm", False), ("lstm", True)}
    assert {c.mode for c in steps} == {"auto", "step", "persist"}
    assert any(c.cell == "lstm" and c.S == 400 and c.B == 33 for c in steps)
    assert any(c.Sc % 16 for c in steps)
    for f in (lambda c: c.O > 64, lambda c: c.L == 1, lambda c: c.T == 1, lambda c: c.L == 17, lambda c: c.B == 17,
              lambda c: c.pen > 0, lambda c: c.pen == 0, lambda c: c.lengths == "ragged"):
        assert any(f(c) for c in steps)
    assert some(lambda c: c.nF > 0 and c.pen > 0 and c.data == "peaked")  # hybrid, peaked, penalty on
    assert some(lambda c: c.path == dc.PERSIST and c.B == 17) and some(lambda c: c.path == dc.PERSIST and c.pen > 0)
    assert some(lambda c: c.path == dc.PERSIST and c.S == 256) and some(lambda c: c.path == dc.XCD and c.S == 256)
    assert some(lambda c: c.dropout > 0 and c.cell == "lstm" and c.nF > 0 and c.path == dc.STEPS)
    assert some(lambda c: c.dropout > 0 and c.path == dc.XCD and c.lengths == "ragged")


@pytest.mark.parametrize("c", [c for c in dc.CASES if c.lengths == "ragged"], ids=lambda c: dc.case_id(c))
def test_ragged_lengths_hold_the_edges(c):
    d = dc.build(c)
    want = {c.L, 1} | ({16} if c.B >= 3 and c.L >= 16 else set()) | ({17} if c.B >= 4 and c.L >= 17 else set())
    assert want <= set(d.flen.tolist()), (want, d.flen)
    if c.nF and c.kW > 1:
        assert (d.flen < c.kW).any()
    assert {c.T, 1} <= set(d.tlen.tolist())
    assert np.abs(d.h[np.arange(c.L)[None, :] >= d.flen[:, None]]).max() > 1.0  # finite garbage on padding frames
    assert not d.dlogp[np.arange(c.T)[None, :] >= d.tlen[:, None]].any()


@pytest.mark.parametrize("c", dc.CASES, ids=IDS)
def test_data_is_float32_and_legs_differ(c):
    d0, d1, d2 = dc.build(c, 0), dc.build(c, 1), dc.build(c, 2)
    assert d0.h.dtype == np.float32 and all(v.dtype == np.float32 for v in d0.P.values())
    assert (d1.L, d1.T) == (max(1, c.L - 3), c.T + 2) and (d2.L, d2.T) == (c.L, max(1, c.T - 1))
    assert all(np.array_equal(d1.P[k], d0.P[k] * np.float32(0.5)) for k in d0.P)
    assert dc.build(c, 3).h is d0.h
    if c.dropout:
        assert set(np.unique(d0.mask).tolist()) == {0.0, 2.0}


@pytest.mark.parametrize("c", [c for c in dc.CASES if c.data == "peaked"], ids=lambda c: dc.case_id(c))
def test_peaked_data_is_peaked(c):
    """(a) max alpha > 0.9 on at least half of the live (b, t); (b) the argmax visits the first chunk and the last,
    ragged one; (c) it changes chunk between two consecutive steps of an utterance; no live alpha underflows."""
    share, chunks, last, moves, span = dc.peaked_stats(c)
    print(f"{dc.case_id(c)}: share {share:.2f}, argmax chunks {sorted(chunks)} of 0..{last}, moves {moves}, "
          f"span {span:.1f}")
    assert share >= 0.5
    assert 0 in chunks and last in chunks and last > 0
    assert dc.build(c).L % dc.chunk_frames(c, c.L) != 0  # the last chunk is ragged
    assert moves
    assert span <= 80.0


def test_plain_data_is_flat():
    """What the peaked cases are for: on the plain twin no (b, t) has max alpha > 0.9 and the scores span < 2."""
    share, _, _, _, span = dc.peaked_stats(dc.CASES[0])
    assert share == 0.0 and span < 2.0


@pytest.mark.parametrize("c", dc.CASES, ids=IDS)
def test_few_decisions_sit_inside_the_margins(c):
    for leg in LEGS:
        nm, close_m, nmono, close_mono = dc.decision_counts(dc.reference(c, leg))
        assert close_m <= dc.MAXOUT_CAP * nm, (leg, close_m, nm)
        if c.pen > 0:
            assert close_mono <= dc.MONO_CAP * nmono, (leg, close_mono, nmono)


@pytest.mark.parametrize("c", dc.CASES, ids=IDS)
def test_floor_makes_the_bar_tight_and_another_order_stays_inside(c):
    """16 x floor < 1e-4 max|ref| for every tensor (the case's `loose` names the tensors where it may not be),
    and the ChunkedK restatement stays within a quarter of the bar built from the plain floor alone."""
    loose = set()
    for leg in LEGS:
        r64, p32, c32 = dc.reference(c, leg), dc.reference(c, leg, np.float32), dc.reference(c, leg, np.float32, True)
        for k, ref in r64.tensors.items():
            scale = float(np.abs(ref).max())
            if scale == 0.0:
                continue
            floor = dc.floor_of(k, r64, dc.restatements(c, leg))
            if not dc.FLOOR_FACTOR * floor < dc.RTOL * scale:
                loose.add(k)
                print(f"{dc.case_id(c)} leg {leg} {k}: floor {floor:.2e} / max|ref| {scale:.2e} = {floor / scale:.2e}")
            plain = float(np.abs(p32.tensors[k] - ref).max())
            other = float(np.abs(np.asarray(c32.tensors[k], np.float64) - ref).max())
            bar = min(dc.FLOOR_FACTOR * plain, dc.RTOL * scale)
            assert 4 * other <= bar, (leg, k, other, plain, scale)
    assert loose <= set(c.loose), sorted(loose)


@pytest.mark.parametrize("fault", dc.FAULTS)
def test_checker_rejects_the_planted_fault(fault):
    cases = [c for c in dc.CASES if dc.fault_applies(c, fault)]
    assert len(cases) >= 3, [dc.case_id(c) for c in cases]
    if fault in ("chunk_max_first", "halo_off_by_one"):
        assert any(c.data == "peaked" for c in cases)
    for c in cases:
        _, fails = dc.check_all(dc.as_got(dc.reference(c, 0, np.float64, False, fault)), c, 0, f" {fault}")
        assert fails, f"{fault} passes on {dc.case_id(c)}"


def test_chunk_max_first_passes_the_flat_bar_on_plain_data():
    """The evidence that the plain data was blind to it: on the plain twin of the first peaked case every argmax
    sits in chunk 0, the fault changes nothing, and the suite's earlier flat bar (1e-4 max|ref|) accepts it."""
    plain, peaked = dc.CASES[0], dc.CASES[1]
    assert plain._replace(data="peaked", note="") == peaked._replace(note="")
    r = dc.reference(plain)
    bad = dc._chunk_max_first(r.tensors["alpha"], 16)
    assert np.abs(bad - r.tensors["alpha"]).max() <= dc.RTOL * np.abs(r.tensors["alpha"]).max()
    rp = dc.reference(peaked)
    badp = dc.reference(peaked, 0, np.float64, False, "chunk_max_first").tensors["alpha"]
    assert np.abs(badp - rp.tensors["alpha"]).max() > 100 * dc.RTOL * np.abs(rp.tensors["alpha"]).max()


def test_checker_accepts_the_reference_a_zero_reference_and_rejects_nan():
    c = dc.CASES[0]
    r = dc.reference(c)
    ratios, fails = dc.check_all(dc.as_got(r), c)
    assert not fails and max(ratios.values()) == 0.0
    z = np.zeros((3, 4))
    assert dc.check(z, z, 0.0, "zero") == (0.0, None)
    assert dc.check(z + 1e-6, z, 0.0, "zero")[1] is not None
    got = dc.as_got(r)
    got["dh"] = got["dh"].copy()
    got["dh"][0, 0, 0] = np.nan
    assert any("non-finite" in m for m in dc.check_all(got, c)[1])
    got = dc.as_got(r)  # a winner flipped outside the margin
    b, t, m = np.argwhere(r.margin > 10 * dc.MAXOUT_MARGIN * r.umax)[0]
    got["maxout_argmax"] = r.winners.copy()
    got["maxout_argmax"][b, t, m] = (r.winners[b, t, m] + 1) % c.K
    assert any("Maxout" in m for m in dc.check_all(got, c)[1])
