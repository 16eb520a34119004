"""CPU: the cases of tests/gemm_case.py are what the GPU tests of the fp32 GEMM family take them for, and the test
entry points report bad arguments instead of aborting."""
import ctypes

import numpy as np
import pytest

import gemm_case as gc


def test_exact_cases_are_exact_in_fp32_in_any_summation_order():
    """What makes a bitwise comparison legitimate: for every exact case of the GPU tables, the expression evaluated in
    numpy float32 -- whole, and in K slices of 32, 256 and 352 summed afterwards (one K-tile, the split-K slice, the
    short-workspace slice) -- equals the float64 reference bit for bit, and the reference is an fp32 number."""
    args = gc.exact_case_args()
    assert len(args) > 400
    for tA, tB, kw in args:
        c = gc.build_case(tA, tB, **kw)
        r32 = c.ref.astype(np.float32)
        assert np.array_equal(r32.astype(np.float64), c.ref), (tA, tB, kw)
        assert not np.isnan(c.ref).any()
        for ks in (0, 32, 256, 352):
            got = gc.reference(c, np.float32, kslice=ks)
            assert got.dtype == np.float32 and np.array_equal(gc.bits(got), gc.bits(r32)), (tA, tB, kw, ks)
        if c.M and c.N and c.K:  # non-zero data: every term counts
            assert np.all(c.opA != 0) and np.all(c.opB != 0) and np.all(c.C0 != 0)


def test_bf16_exact_cases_are_bf16_numbers_and_exact_in_any_order():
    """The bf16 families' exact cases: every operand value is a bf16 number already (bf16_round(x) == x, so the
    kernels' rounding cannot touch it: build_case asserts it, and it is asserted here again), and the expression in
    fp32 -- whole, and in K slices of one K-tile (64) and of the split table's slices -- is the float64 reference bit
    for bit."""
    args = gc.bf16_exact_case_args()
    assert len(args) > len(gc.exact_case_args())
    for tA, tB, kw in args:
        c = gc.build_case(tA, tB, precision="bf16", **kw)
        for x in (c.opA, c.opB):
            assert np.array_equal(gc.bits(gc.bf16_round(x)), gc.bits(x)), (tA, tB, kw)
        r32 = c.ref.astype(np.float32)
        assert np.array_equal(r32.astype(np.float64), c.ref) and not np.isnan(c.ref).any(), (tA, tB, kw)
        if max(c.M, c.N) > 2048:
            continue  # the wide 64 x 128 shapes: K <= 100, the slices below are the whole product
        for ks in (0, 64, 256, 384, 448):
            got = gc.reference(c, np.float32, kslice=ks)
            assert np.array_equal(gc.bits(got), gc.bits(r32)), (tA, tB, kw, ks)


def _rounding_cases():
    return [gc.build_case(tA, tB, data="rounding", precision="bf16", **kw) for tA, tB in gc.FORMS for kw in gc.BF16_ROUNDING]


def test_rounding_values_are_what_the_leg_says():
    v = gc.ROUNDING_VALUES
    r = gc.bf16_round(v)
    assert v.size == 40 and np.all(r != v)  # none is a bf16 number
    assert np.array_equal(r * 128, np.round(r * 128)) and np.abs(r).max() == 4  # multiples of 2^-7, magnitude <= 4
    p = np.array(gc.ROUNDING_PATTERNS, dtype=np.float32)
    rp = gc.bf16_round(p).astype(np.float64)
    want = [1, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1.5, 1.75 + 2.0 ** -6, 2, 2]
    assert rp.tolist() == want
    # ties go both ways, and the three wrong roundings each move some value
    assert (rp < p).any() and (rp > p).any()
    for wrong in (gc.bf16_truncate, gc.bf16_round_ties_away):
        assert np.any(wrong(v) != r)


def test_rounding_leg_is_exact_in_fp32_and_tells_rne_from_other_roundings():
    """The rounding leg's cases: the bound holds (build_case asserts it; here the fp32 sums in two orders and in
    slices equal the float64 product of the rounded operands bit for bit), and the same data gives different expected
    bits under truncation, ties away from zero and no rounding at all -- in a large share of the elements, so a kernel
    with any of them fails the bitwise comparison."""
    for c in _rounding_cases():
        r32 = c.ref.astype(np.float32)
        assert np.array_equal(r32.astype(np.float64), c.ref)
        for ks in (0, 32, 8):
            assert np.array_equal(gc.bits(gc.reference(c, np.float32, kslice=ks)), gc.bits(r32))
        back = gc.reference(c, np.float32, opA=c.mulA[:, ::-1], opB=c.mulB[::-1])  # the other summation order
        assert np.array_equal(gc.bits(back), gc.bits(r32))
        for name, f in (("truncation", gc.bf16_truncate), ("ties away", gc.bf16_round_ties_away), ("none", lambda x: x)):
            other = gc.reference(c, np.float64, opA=f(c.opA), opB=f(c.opB))
            differ = float(np.mean(other != c.ref))
            assert differ > 0.25, (name, c.M, c.N, c.K, differ)  # (a ReLU case: about half its elements are 0)


def test_200_rounding_draws_at_k64_are_exact_in_two_orders():
    rng = np.random.default_rng(64)
    for _ in range(200):
        a = gc.bf16_round(rng.choice(gc.ROUNDING_VALUES, size=(8, 64)).astype(np.float32))
        b = gc.bf16_round(rng.choice(gc.ROUNDING_VALUES, size=(64, 8)).astype(np.float32))
        ref = a.astype(np.float64) @ b.astype(np.float64)
        fwd = np.zeros((8, 8), np.float32)
        bwd = np.zeros((8, 8), np.float32)
        for k in range(64):
            fwd = fwd + a[:, k:k + 1] * b[k:k + 1]
            bwd = bwd + a[:, 63 - k:64 - k] * b[63 - k:64 - k]
        assert fwd.dtype == np.float32 and np.array_equal(fwd.astype(np.float64), ref)
        assert np.array_equal(bwd.astype(np.float64), ref)


def test_bf16_split_table_follows_the_halving_rule():
    """The split table and the wide-tile table are what plan_gemm's bf16 branch, restated in gc.bf16_tile_plan, gives
    (the GPU tests assert the same values from the library's own record): 2, 4, 8 and 16 slices, a ragged last slice,
    and slices that are not a power of two."""
    for M, N, K, s, ks in gc.BF16_SPLIT_SWEEP:
        assert gc.bf16_tile_plan([(M, N, K)], gc.BF16_WS_FLOATS) == (64, 64, ks, s, [s]), (M, N, K)
    counts = {s for _, _, _, s, _ in gc.BF16_SPLIT_SWEEP}
    assert {2, 4, 8, 16} <= counts
    assert any(K % ks for _, _, K, _, ks in gc.BF16_SPLIT_SWEEP)  # a ragged last slice
    assert (60, 45, 768, 2, 384) in gc.BF16_SPLIT_SWEEP  # a slice that is no power of two
    for M, N, K, bm, bn in gc.BF16_WIDE_TILES:
        got = gc.bf16_tile_plan([(M, N, K)], gc.BF16_WS_FLOATS)
        assert got[:3] == (bm, bn, (K + 63) // 64 * 64) and got[3] >= 256 and got[4] == [1], (M, N, K, got)
    # without a workspace nothing splits; the wider tile is not taken below 256 tiles
    assert gc.bf16_tile_plan([(60, 45, 4096)], 0)[2:] == (4096, 1, [1])
    assert gc.bf16_tile_plan([(2048, 1920, 64)], gc.BF16_WS_FLOATS)[:2] == (64, 64)


def test_windows_are_placed_as_documented():
    for aligned in (False, True):
        c = gc.build_case(1, 0, 40, 64, 96, Mread=64, bias=True, rbias=True, beta=0.0, aligned=aligned)
        for w in (c.A, c.B, c.C, c.bias, c.rbias):
            if aligned:
                assert w.off % 4 == 0 and w.ld % 4 == 0 and w.ld > w.cols
            else:
                assert w.off % 2 == 1 and w.ld % 2 == 1 and w.ld > w.cols
            assert w.index().max() < w.buf.size
        for w in (c.A, c.B, c.bias, c.rbias):  # inputs: NaN outside the window, none inside
            assert np.isnan(w.buf[w.outside()]).all() and not np.isnan(w.get()).any()
        a = c.A.get()  # transposed form: K x Mread, the declared padding is zeros
        assert a.shape == (96, 64) and np.all(a[:, 40:] == 0) and np.all(a[:, :40] != 0)
        assert np.array_equal(a[:, :40].T, c.opA)
        assert np.all(gc.bits(c.C.buf[c.C.outside()]) == gc.CANARY)
        assert np.isnan(c.C.get()).all()  # beta == 0: C0 must not be read
        assert np.array_equal(gc.bits(c.expect[c.C.outside()]), gc.bits(c.C.buf[c.C.outside()]))
    # the same problem with and without the padded-read declaration
    p = gc.build_case(0, 1, 64, 40, 96, Nread=64)
    q = gc.build_case(0, 1, 64, 40, 96)
    assert np.array_equal(p.ref, q.ref) and p.B.rows == 64 and q.B.rows == 40
    assert np.all(p.B.get()[40:] == 0)


def test_precision_bar_separates_fp32_from_bf16_operands():
    """The precision leg's bar must not pass a kernel that rounds its operands: the float64 reference recomputed from
    bf16-rounded A and B misses the bar by at least 5x on every precision case."""
    for tA, tB, kw in gc.precision_case_args():
        c = gc.build_case(tA, tB, **kw)
        low = gc.reference(c, np.float64, opA=gc.bf16_round(c.opA), opB=gc.bf16_round(c.opB))
        miss = np.abs(low - c.ref).max() / np.abs(c.ref).max()
        assert miss >= 5 * gc.PRECISION_BAR, (kw, miss)


def test_debug_entries_report_bad_arguments():
    """0 and 17 problems for the batch entry, 25 ranges for the colsum_scatter entry: an error code and a message, no
    abort.  Every call fails its checks on the host, before any device call; no pointer below is dereferenced."""
    from s2s_amd import _lib
    lib = _lib.lib
    e = gc.declare(lib)
    probs = (e.Problem * 17)()
    plan = e.Plan()
    for n in (0, 17, -1):
        assert lib.s2s_debug_gemm_batch(None, probs, n, 0, 0, None, 0, ctypes.byref(plan)) != 0
        assert "debug_gemm_batch" in lib.s2s_last_error().decode()
    assert lib.s2s_debug_gemm_batch(None, None, 1, 0, 0, None, 0, ctypes.byref(plan)) != 0
    assert "null" in lib.s2s_last_error().decode()
    assert lib.s2s_debug_gemm_batch(None, probs, 1, 0, 0, None, 0, None) != 0
    assert "null" in lib.s2s_last_error().decode()
    assert lib.s2s_debug_gemm_batch_prec(None, probs, 17, 0, 0, 1, None, 0, ctypes.byref(plan)) != 0
    assert "debug_gemm_batch" in lib.s2s_last_error().decode()
    # the big-tile GEMM's test override takes the three tiles it is built for and 0 .. 256 slices, nothing else
    try:
        for bm, bn, s in ((128, 64, 0), (64, 64, 0), (128, 256, 0), (256, 0, 0), (0, 0, 257), (0, 0, -1), (128, 128, 1000)):
            assert lib.s2s_debug_gemm_big_force(bm, bn, s) != 0, (bm, bn, s)
        for bm, bn, s in ((256, 256, 0), (256, 128, 3), (128, 128, 256), (0, 0, 2)):
            assert lib.s2s_debug_gemm_big_force(bm, bn, s) == 0, (bm, bn, s)
    finally:  # whatever failed above, no override stays behind on this thread
        assert lib.s2s_debug_gemm_big_force(0, 0, 0) == 0
    outs = (e.ColsumOut * 25)()
    fake = ctypes.c_void_p(4096)
    assert lib.s2s_debug_colsum_scatter(None, fake, 8, 4, 8, 1.0, outs, 25, None, 0) != 0
    assert "colsum_scatter" in lib.s2s_last_error().decode()
    # a bad range or destination count is refused in the one-stage form too (no workspace), before anything runs
    for col0, ncols, ndst in ((0, 4, 4), (6, 4, 1), (-1, 4, 1), (0, 4, -1)):
        outs[0].col0, outs[0].ncols, outs[0].ndst = col0, ncols, ndst
        assert lib.s2s_debug_colsum_scatter(None, fake, 8, 4, 8, 1.0, outs, 1, None, 0) != 0
        assert "bad range" in lib.s2s_last_error().decode()
