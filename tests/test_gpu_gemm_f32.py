"""GPU: the fp32 MFMA GEMM and its helpers (csrc/gemm_f32.hip) tested directly, against float64, through the test
entry points of csrc/capi_debug.cpp (s2s_debug_gemm_batch and one entry per helper).

The cases come from tests/gemm_case.py: operands and outputs are windows at odd offsets with odd leading dimensions
inside NaN-filled (inputs) or canary-filled (outputs) arrays, and the data is exact -- small non-zero integers, so
the fp32 result is the float64 reference whatever the summation order.  Every exact check is therefore bitwise, on
the whole output array: the result inside the window and the canary around it.  Split-K tests assert the split count
and slice length the library reports for the launch it made (GemmLastPlan), so a planner change cannot turn them
into unsplit tests unnoticed.  Only the precision leg (random normal data) has a tolerance: the project's own
max|gpu - ref| <= 2e-5 max|ref|; it prints the measured ratio of every case.
"""
import numpy as np
import pytest
import torch

import gemm_case as gc
from gemm_gpu import WS_FLOATS, load, run_batch, run_exact  # the runner the bf16 tests share
from gemm_gpu import dev as _dev, ok as _ok, ptr as _ptr, same_bits as _same_bits, stream as _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def s2s():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load()


def _tiles(c):
    return ((c.M + 63) // 64) * ((c.N + 63) // 64)


def _assert_unsplit(plan, c):
    assert (plan.launched, plan.bm, plan.bn, plan.reduced) == (1, 64, 64, 0)
    assert plan.splits[0] == 1 and plan.nblocks == _tiles(c)


# ------------------------------------------------------------------------------------------------ the tile kernel
@pytest.mark.parametrize("tA,tB", gc.FORMS)
@pytest.mark.parametrize("M,N,K", gc.SINGLE_SHAPES)
def test_tile_kernel_exact(s2s, tA, tB, M, N, K):
    """Whole and ragged tiles, the K tail of a fast tile, K below one K-tile, 9 and 17 blocks over the XCD remap."""
    c = gc.build_case(tA, tB, M, N, K)
    _, plan = run_exact(s2s, c, with_ws=False)
    _assert_unsplit(plan, c)


@pytest.mark.parametrize("tA,tB", gc.FORMS)
@pytest.mark.parametrize("opt", gc.K0_OPTIONS, ids=lambda o: f"bias{int(o['bias'])}-beta{o['beta']}")
def test_k_zero_gives_beta_c_plus_bias(s2s, tA, tB, opt):
    c = gc.build_case(tA, tB, 40, 33, 0, **opt)
    _, plan = run_exact(s2s, c)
    _assert_unsplit(plan, c)


@pytest.mark.parametrize("tA,tB", gc.FORMS)
@pytest.mark.parametrize("M,N,K", gc.EMPTY_SHAPES)
def test_empty_output_launches_nothing(s2s, tA, tB, M, N, K):
    c = gc.build_case(tA, tB, M, N, K, beta=1.0)
    _, plan = run_exact(s2s, c)
    assert plan.launched == 0 and plan.splits[0] == 0


@pytest.mark.parametrize("tA,tB", gc.FORMS)
@pytest.mark.parametrize("kw", gc.PADDED, ids=("Nread", "Mread"))
def test_padded_reads(s2s, tA, tB, kw):
    """Mread / Nread let the ragged tile take the unguarded loads over the caller's zero padding (rows of a
    K-contiguous operand, columns of a row-contiguous one: both forms are among the four): the result is exact, and
    bitwise the result of the same problem without the declaration."""
    c = gc.build_case(tA, tB, **kw)
    plain = gc.build_case(tA, tB, **dict(kw, Mread=0, Nread=0))
    out, plan = run_exact(s2s, c, with_ws=False)
    out_plain, _ = run_exact(s2s, plain, with_ws=False)
    _assert_unsplit(plan, c)
    assert np.array_equal(gc.bits(c.C.get(out)), gc.bits(plain.C.get(out_plain)))


@pytest.mark.parametrize("tA,tB", gc.FORMS)
@pytest.mark.parametrize("i", range(len(gc.EPILOGUES)))
def test_direct_epilogue(s2s, tA, tB, i):
    M, N, K = gc.EPILOGUE_SHAPE
    c = gc.build_case(tA, tB, M, N, K, **gc.EPILOGUES[i])
    _, plan = run_exact(s2s, c, with_ws=False)
    _assert_unsplit(plan, c)


@pytest.mark.parametrize("tA,tB", gc.FORMS)
def test_single_problem_entry_fp32(s2s, tA, tB):
    """s2s_debug_gemm(bf16 = 0): the same kernels through the older single-problem entry."""
    c = gc.build_case(tA, tB, 77, 45, 133, alpha=0.5, beta=0.25)
    a, b, cd = _dev(c.A.buf), _dev(c.B.buf), _dev(c.C.buf)
    rc = s2s.lib.s2s_debug_gemm(tA, tB, c.M, c.N, c.K, c.alpha, _ptr(a, c.A.off), c.A.ld, _ptr(b, c.B.off), c.B.ld,
                                c.beta, _ptr(cd, c.C.off), c.C.ld, 0, s2s.ws.data_ptr(), WS_FLOATS)
    _ok(s2s, rc)
    torch.cuda.synchronize()
    _same_bits(cd.cpu().numpy(), c.expect, c.C, "s2s_debug_gemm")


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
@pytest.mark.parametrize("M,N,K,s", gc.SPLIT_SWEEP)
def test_splitk_every_slab_count(s2s, tA, tB, M, N, K, s):
    """One output tile cut into s slices of 256 (the last one ragged for K = 256 s - 5): every tail 1..7 of
    slab_sum's switch behind 0, 1, 2 and 3 groups of 8.  Two runs are bitwise equal."""
    c = gc.build_case(tA, tB, M, N, K)
    out, plan = run_exact(s2s, c)
    assert (plan.launched, plan.bm, plan.bn, plan.reduced) == (1, 64, 64, 1)
    assert plan.splits[0] == s and plan.kslice == 256 and plan.nblocks == s
    again, plan2 = run_exact(s2s, c)
    assert plan2.splits[0] == s and np.array_equal(gc.bits(out), gc.bits(again))


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
@pytest.mark.parametrize("s", gc.SPLIT_EPILOGUE_COUNTS)
@pytest.mark.parametrize("M,N,aligned", gc.SPLIT_EPILOGUE_SHAPES, ids=("f4slab_f4c", "f4slab_scalarc", "scalar"))
def test_splitk_reduce_epilogues(s2s, tA, tB, s, M, N, aligned):
    """Every epilogue flag through each of splitk_reduce's three paths (the path follows from M N % 4, N % 4,
    ldc % 4 and the alignment of the slabs and of C, asserted here)."""
    for opt in gc.EPILOGUES:
        c = gc.build_case(tA, tB, M, N, 256 * s, aligned=aligned, **opt)
        if aligned:
            assert M * N % 4 == 0 and N % 4 == 0 and c.C.ld % 4 == 0 and c.C.off % 4 == 0
        elif M * N % 4 == 0:
            assert N % 4 != 0 and c.C.ld % 4 != 0
        else:
            assert M * N % 2 == 1
        _, plan = run_exact(s2s, c)
        assert plan.splits[0] == s and plan.kslice == 256 and plan.reduced == 1, opt


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
def test_short_workspace_limits_the_split(s2s, tA, tB):
    """Slabs must fit the workspace: exactly 3 M N floats give 3 slices (of 352), a pointer with 0 floats none."""
    M, N, K = gc.SHORT_WS
    c = gc.build_case(tA, tB, M, N, K)
    _, plan = run_exact(s2s, c, ws_floats=3 * M * N)
    assert plan.splits[0] == 3 and plan.kslice == 352 and plan.reduced == 1
    _, plan = run_exact(s2s, c, ws_floats=0)
    _assert_unsplit(plan, c)
    _, plan = run_exact(s2s, c, with_ws=False)
    _assert_unsplit(plan, c)


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
def test_multi_tile_split(s2s, tA, tB):
    M, N, K = gc.MULTI_TILE_SPLIT
    c = gc.build_case(tA, tB, M, N, K)
    _, plan = run_exact(s2s, c)
    assert plan.splits[0] == 4 and plan.kslice == 256 and plan.nblocks == 4 * 9 and plan.reduced == 1


# ------------------------------------------------------------------------------------------------ batches
def _batch_alone_and_together(s2s, cases, splits):
    outs, plan = run_batch(s2s, cases)
    assert list(plan.splits[:len(cases)]) == splits
    for i, (c, out) in enumerate(zip(cases, outs)):
        _same_bits(out, c.expect, c.C, f"problem {i} of the batch")
    return plan


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
def test_mixed_batch(s2s, tA, tB):
    """Two split problems (the second one's slabs start at an odd float offset behind the first's 7 x 33 x 45, so it
    takes the scalar reduce although its M N % 4 == 0), one unsplit problem written by the tile kernel, one with
    K = 0 and one skipped, each with its own epilogue, in one call: every C and canary exact -- which no problem's
    could be if it depended on its neighbours."""
    cases = [gc.build_case(tA, tB, **kw) for kw in gc.MIXED_BATCH]
    assert (7 * cases[0].M * cases[0].N) % 2 == 1
    plan = _batch_alone_and_together(s2s, cases, [7, 7, 1, 1, 0])
    assert plan.kslice == 256 and plan.reduced == 1 and plan.nblocks == 7 + 7 + 1 + 1
    # the second problem alone: now its slabs are aligned (the float4 reduce); same bits
    alone, plan = run_exact(s2s, cases[1])
    assert plan.splits[0] == 7


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
def test_sixteen_problems_in_one_call(s2s, tA, tB):
    cases = [gc.build_case(tA, tB, **kw) for kw in gc.SIXTEEN]
    plan = _batch_alone_and_together(s2s, cases, [1] * 16)
    assert plan.nblocks == sum(_tiles(c) for c in cases) and plan.reduced == 0


# ------------------------------------------------------------------------------------------------ precision
@pytest.mark.parametrize("tA,tB,kw", gc.precision_case_args(),
                         ids=lambda v: f"{v['M']}x{v['N']}x{v['K']}" if isinstance(v, dict) else str(v))
def test_precision_on_random_data(s2s, tA, tB, kw):
    """Standard normal operands against float64 at the bar of the bf16 kernels' exactness test (the same fp32
    accumulation in the same tile order, and here no operand rounding): max|gpu - ref| <= 2e-5 max|ref|."""
    c = gc.build_case(tA, tB, **kw)
    (out,), plan = run_batch(s2s, [c])
    if c.K == 8192:
        assert plan.splits[0] == 32 and plan.reduced == 1
    if c.K == 4352:
        assert plan.splits[0] == 17 and plan.reduced == 1
    ratio = np.abs(c.C.get(out).astype(np.float64) - c.ref).max() / np.abs(c.ref).max()
    print(f"precision ({tA},{tB}) {c.M}x{c.N}x{c.K} splits {plan.splits[0]}: max|gpu-ref|/max|ref| = {ratio:.3e} "
          f"({ratio / gc.PRECISION_BAR:.3f} of the bar)")
    out_side = c.C.outside()
    assert np.all(gc.bits(out[out_side]) == gc.CANARY)
    assert ratio <= gc.PRECISION_BAR, ratio


# ------------------------------------------------------------------------------------------------ helpers
def _ints(rng, shape):
    return gc.draw(rng, shape, True)


NAN = np.float32(np.nan)
COLSUM_M = tuple(range(1, 41)) + tuple(range(120, 201)) + (4096, 4097, 4163)


def _colsum_expect(X, alpha, beta, out0, prior):
    ref = (beta * prior.astype(np.float64) if beta != 0 else 0.0) + alpha * X.get().astype(np.float64).sum(axis=0)
    assert np.abs(ref).max() < 2 ** 22
    expect = out0.buf.copy()
    expect[out0.index()] = ref.astype(np.float32)
    return expect


@pytest.mark.parametrize("N", (1, 63, 64, 65, 379))
def test_colsum_every_row_count(s2s, N):
    """colsum_f32 one-stage (no workspace) and two-stage: M through 1..40 and 120..200 (colsum_parts changes at 128;
    every residue of the slice length mod 16 in the unrolled loop's tail) and 4096, 4097, 4163 (64 slices); a
    workspace of exactly 64 N floats and a larger one give the same bits, one of 64 N - 1 falls back to one stage."""
    rng = np.random.default_rng(1000 + N)
    for M in COLSUM_M:
        alpha, beta = (0.5, -2.0, 0.25)[M % 3], (0.0, 1.0, 0.5)[(M // 3) % 3]
        X = gc.Win(M, N, NAN).put(_ints(rng, (M, N)))
        prior = _ints(rng, (1, N))
        out0 = gc.Win(1, N, gc.canary_f32()).put(prior if beta != 0 else np.full((1, N), NAN))
        expect = _colsum_expect(X, alpha, beta, out0, prior)
        xd = _dev(X.buf)
        outs = []
        for ws_n in (None, 64 * N, 64 * N + 1000, 64 * N - 1):
            od = _dev(out0.buf)
            _ok(s2s, s2s.lib.s2s_debug_colsum(_stream(), _ptr(xd, X.off), X.ld, M, N, alpha, beta, _ptr(od, out0.off),
                                              None if ws_n is None else s2s.ws.data_ptr(), ws_n or 0))
            outs.append(od)
        torch.cuda.synchronize()
        for od, name in zip(outs, ("one stage", "ws = 64 N", "ws > 64 N", "ws = 64 N - 1")):
            _same_bits(od.cpu().numpy(), expect, out0, f"colsum M {M} N {N} alpha {alpha} beta {beta}, {name}")


@pytest.mark.parametrize("M,N", ((200, 65), (4163, 379)))
def test_colsum_two_stage_same_bits_for_any_sufficient_workspace(s2s, M, N):
    """The promise of s2s_common.h on data where the summation order shows (standard normal)."""
    rng = np.random.default_rng(M + N)
    X = gc.Win(M, N, NAN).put(rng.standard_normal((M, N)))
    xd = _dev(X.buf)
    outs = []
    for ws_n in (64 * N, 64 * N + 4096, WS_FLOATS):
        od = _dev(np.full(N + 2, gc.canary_f32()))
        _ok(s2s, s2s.lib.s2s_debug_colsum(_stream(), _ptr(xd, X.off), X.ld, M, N, 0.5, 0.0, _ptr(od, 1),
                                          s2s.ws.data_ptr(), ws_n))
        outs.append(od.cpu().numpy())
    ref = 0.5 * X.get().astype(np.float64).sum(axis=0)
    assert np.abs(outs[0][1:-1] - ref).max() <= 1e-5 * np.abs(ref).max()
    for o in outs:
        _same_bits(o, outs[0], None, "colsum two-stage")
        assert gc.bits(o)[0] == gc.CANARY and gc.bits(o)[-1] == gc.CANARY


def _scatter_ranges(nr, N):
    if nr == 1:
        return [(5, 20)]
    if nr == 3:
        return [(0, 10), (10, 30), (25, N - 25)]  # adjacent, then overlapping, up to the last column
    return [(15 * i, 15 if i % 2 == 0 else 22) for i in range(nr)]  # adjacent and overlapping in turn


@pytest.mark.parametrize("data", ("exact", "random"))
@pytest.mark.parametrize("with_ws", (True, False))
@pytest.mark.parametrize("M", (100, 1000))
@pytest.mark.parametrize("nr", (1, 3, 24))
def test_colsum_scatter_is_colsum_per_range_and_destination(s2s, nr, M, with_ws, data):
    """colsum_scatter_f32 over 1, 3 and 24 ranges with 1..3 destinations holding prior values, with a sufficient
    workspace (two launches for M >= 128) and with none (the per-destination fallback): bitwise colsum_f32(X + col0,
    ..., alpha, 1, dst) on the same workspace -- on exact data also the float64 sums, on normal data the promise
    itself, where the order of summation shows."""
    N, alpha = 379, 0.5
    rng = np.random.default_rng(nr + M)
    X = gc.Win(M, N, NAN).put(_ints(rng, (M, N)) if data == "exact" else rng.standard_normal((M, N)))
    xd = _dev(X.buf)
    ranges = _scatter_ranges(nr, N)
    assert all(c0 >= 0 and c0 + nc <= N for c0, nc in ranges)
    outs = (s2s.ColsumOut * nr)()
    dst = []  # (window, prior, scatter's array, colsum's array, col0)
    for e, (c0, nc) in enumerate(ranges):
        outs[e].col0, outs[e].ncols, outs[e].ndst = c0, nc, 1 + e % 3
        for q in range(outs[e].ndst):
            prior = _ints(rng, (1, nc))
            w = gc.Win(1, nc, gc.canary_f32()).put(prior)
            d1, d2 = _dev(w.buf), _dev(w.buf)
            outs[e].dst[q] = _ptr(d1, w.off)
            dst.append((w, prior, d1, d2, c0))
    wsp, wsn = (s2s.ws.data_ptr(), WS_FLOATS) if with_ws else (None, 0)
    _ok(s2s, s2s.lib.s2s_debug_colsum_scatter(_stream(), _ptr(xd, X.off), X.ld, M, N, alpha, outs, nr, wsp, wsn))
    for w, prior, d1, d2, c0 in dst:
        _ok(s2s, s2s.lib.s2s_debug_colsum(_stream(), _ptr(xd, X.off + c0), X.ld, M, w.cols, alpha, 1.0,
                                          _ptr(d2, w.off), wsp, wsn))
    torch.cuda.synchronize()
    for w, prior, d1, d2, c0 in dst:
        got = d1.cpu().numpy()
        _same_bits(got, d2.cpu().numpy(), w, f"scatter vs colsum, range at {c0}")
        assert np.all(gc.bits(got[w.outside()]) == gc.CANARY)
        if data == "exact":
            Xw = gc.Win(M, w.cols, NAN)
            Xw.buf, Xw.off, Xw.ld = X.buf, X.off + c0, X.ld
            _same_bits(got, _colsum_expect(Xw, alpha, 1.0, w, prior), w, f"scatter vs float64, range at {c0}")


def test_transpose(s2s):
    rng = np.random.default_rng(5)
    for rows in (1, 31, 32, 33, 70):
        for cols in (1, 31, 32, 33, 70):
            src = gc.Win(rows, cols, NAN).put(_ints(rng, (rows, cols)))
            dst = gc.Win(cols, rows, gc.canary_f32()).put(np.full((cols, rows), NAN))
            expect = dst.buf.copy()
            expect[dst.index()] = src.get().T
            sd, dd = _dev(src.buf), _dev(dst.buf)
            _ok(s2s, s2s.lib.s2s_debug_transpose(_stream(), _ptr(sd, src.off), src.ld, rows, cols, _ptr(dd, dst.off),
                                                 dst.ld))
            _same_bits(dd.cpu().numpy(), expect, dst, f"transpose {rows} x {cols}")


@pytest.mark.parametrize("acc", (0, 1))
@pytest.mark.parametrize("rows,cols", ((1, 1), (7, 379), (1030, 513)))  # the last: > 2048 x 256 elements, grid-stride
def test_copy2d(s2s, rows, cols, acc):
    rng = np.random.default_rng(rows + cols)
    src = gc.Win(rows, cols, NAN).put(_ints(rng, (rows, cols)))
    prior = _ints(rng, (rows, cols))
    dst = gc.Win(rows, cols, gc.canary_f32()).put(prior if acc else np.full((rows, cols), NAN))
    expect = dst.buf.copy()
    expect[dst.index()] = src.get() + prior if acc else src.get()
    sd, dd = _dev(src.buf), _dev(dst.buf)
    _ok(s2s, s2s.lib.s2s_debug_copy2d(_stream(), _ptr(sd, src.off), src.ld, _ptr(dd, dst.off), dst.ld, rows, cols, acc))
    _same_bits(dd.cpu().numpy(), expect, dst, "copy2d")


@pytest.mark.parametrize("rows,cols,dcols,wide", ((7, 5, 12, True), (9, 5, 8, False), (7, 12, 12, True),
                                                  (2100, 200, 260, True)))  # the last: past the grid-stride bound
def test_pad_cols(s2s, rows, cols, dcols, wide):
    """cols < dcols and cols == dcols, source rows longer than cols (wide) or dense; dst is dense rows x dcols."""
    rng = np.random.default_rng(rows + dcols)
    src = gc.Win(rows, cols, NAN).put(_ints(rng, (rows, cols)))
    if not wide:  # lds == cols: a dense source
        src.ld = cols
        src.buf[:] = NAN
        src.put(_ints(rng, (rows, cols)))
    dst = gc.Win(1, rows * dcols, gc.canary_f32()).put(np.full((1, rows * dcols), NAN))
    want = np.zeros((rows, dcols), np.float32)
    want[:, :cols] = src.get()
    expect = dst.buf.copy()
    expect[dst.index()] = want.reshape(1, -1)
    sd, dd = _dev(src.buf), _dev(dst.buf)
    _ok(s2s, s2s.lib.s2s_debug_pad_cols(_stream(), _ptr(sd, src.off), src.ld, _ptr(dd, dst.off), rows, cols, dcols))
    _same_bits(dd.cpu().numpy(), expect, dst, "pad_cols")


@pytest.mark.parametrize("beta", (0.0, 0.5))
@pytest.mark.parametrize("n", (1, 255, 257, 2048 * 256 + 3))
def test_axpby(s2s, n, beta):
    """beta = 0 overwrites a NaN destination; n past 2048 x 256 reaches the grid-stride loop."""
    rng = np.random.default_rng(n)
    alpha = -2.0
    src = gc.Win(1, n, NAN).put(_ints(rng, (1, n)))
    prior = _ints(rng, (1, n))
    dst = gc.Win(1, n, gc.canary_f32()).put(prior if beta != 0 else np.full((1, n), NAN))
    expect = dst.buf.copy()
    expect[dst.index()] = alpha * src.get() + (beta * prior if beta != 0 else 0)
    sd, dd = _dev(src.buf), _dev(dst.buf)
    _ok(s2s, s2s.lib.s2s_debug_axpby(_stream(), _ptr(sd, src.off), _ptr(dd, dst.off), n, alpha, beta))
    _same_bits(dd.cpu().numpy(), expect, dst, "axpby")


@pytest.mark.parametrize("count", (0, 1, 2048 * 256 + 5))
def test_fill_and_zero(s2s, count):
    """fill_u32_async / zero_async write their range and nothing beside it; a count of 0 is a no-op."""
    pad = 7
    host = np.full(count + 2 * pad, gc.canary_f32(), dtype=np.float32)
    for value, call in ((0x12345678, lambda d: s2s.lib.s2s_debug_fill_u32(_stream(), _ptr(d, pad), 0x12345678, count)),
                        (0, lambda d: s2s.lib.s2s_debug_zero(_stream(), _ptr(d, pad), 4 * count))):
        d = _dev(host)
        _ok(s2s, call(d))
        got = gc.bits(d.cpu().numpy())
        assert np.all(got[:pad] == gc.CANARY) and np.all(got[pad + count:] == gc.CANARY)
        assert np.all(got[pad:pad + count] == value)
