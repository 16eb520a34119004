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
    outs = (e.ColsumOut * 25)()
    fake = ctypes.c_void_p(4096)
    assert lib.s2s_debug_colsum_scatter(None, fake, 8, 4, 8, 1.0, outs, 25, None, 0) != 0
    assert "colsum_scatter" in lib.s2s_last_error().decode()
    # a bad range or destination count is refused in the one-stage form too (no workspace), before anything runs
    for col0, ncols, ndst in ((0, 4, 4), (6, 4, 1), (-1, 4, 1), (0, 4, -1)):
        outs[0].col0, outs[0].ncols, outs[0].ndst = col0, ncols, ndst
        assert lib.s2s_debug_colsum_scatter(None, fake, 8, 4, 8, 1.0, outs, 1, None, 0) != 0
        assert "bad range" in lib.s2s_last_error().decode()
