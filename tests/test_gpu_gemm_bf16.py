"""GPU: the bf16-operand kernels tested directly and bitwise, against float64 -- gemm_bf16_kernel<TA, TB, BM, BN>
(csrc/gemm_f32.hip), the big-tile GEMM (csrc/gemm_bf16.hip: two staging kernels, three tiles, its own split-K reduce)
and the implicit convolutions (csrc/conv_bf16.inc).

The harness is the fp32 family's (tests/gemm_case.py, tests/gemm_gpu.py): windows at odd offsets with odd leading
dimensions inside NaN-filled inputs and canary-filled outputs, non-zero integers -4..4 as data.  Those integers are bf16
numbers, so the kernels' operand rounding leaves them alone and the fp32 result is the float64 reference whatever the
order of summation: every comparison is bitwise, on the whole output array.  The rounding leg feeds values that are
not bf16 numbers but round (RNE) to small dyadic ones, with K <= 64, so it is bitwise too and fails under truncation,
ties-away or no rounding.  Every case that names a tile or a split asserts it from the library's own record of the
launch (GemmLastPlan, GemmBigLastPlan); the big-tile GEMM's tiles are reached at small shapes through its test
override (s2s_debug_gemm_big_force), which changes the plan and nothing in the kernels.  Only the precision leg
(normal data) has a tolerance, the project's max|gpu - ref| <= 2e-5 max|ref|.
"""
import ctypes

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view as win

import gemm_case as gc
from gemm_gpu import WS_FLOATS, dev, fill_problem, load, ok, ptr, run_batch, run_exact, same_bits, stream

pytestmark = pytest.mark.gpu

RC, KC_SCALAR, KC_VEC = 0, 1, 2  # kStageRc, kStageKcScalar, kStageKcVec


@pytest.fixture(scope="module")
def s2s():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = load()
    assert WS_FLOATS == gc.BF16_WS_FLOATS
    return e


def bf(tA, tB, M=None, N=None, K=None, **kw):
    return gc.build_case(tA, tB, M, N, K, precision="bf16", **kw)


def _assert_plan(plan, cases, ws_floats=WS_FLOATS):
    """The record of the launch is plan_gemm's bf16 branch for these problems (restated in gc.bf16_tile_plan)."""
    live = [(i, c) for i, c in enumerate(cases) if c.M > 0 and c.N > 0]
    bm, bn, ks, blocks, splits = gc.bf16_tile_plan([(c.M, c.N, c.K) for _, c in live], ws_floats)
    assert (plan.launched, plan.bm, plan.bn, plan.kslice, plan.nblocks) == (1, bm, bn, ks, blocks)
    want = [0] * len(cases)
    for (i, _), s in zip(live, splits):
        want[i] = s
    assert list(plan.splits[:len(cases)]) == want
    assert plan.reduced == int(any(s > 1 for s in splits))
    return bm, bn, ks, splits


# ------------------------------------------------------------------------------------------------ the tile family
@pytest.mark.parametrize("tA,tB", gc.FORMS)
@pytest.mark.parametrize("M,N,K", gc.BF16_SINGLE_SHAPES)
def test_tile_kernel_exact(s2s, tA, tB, M, N, K):
    """64 x 64 tiles: whole and ragged, whole 64-deep K-tiles on the unguarded loader, K = 63 / 65 / 100 / 369 tails
    on the guarded one, K below one K-tile, 9 and 17 blocks over the XCD remap."""
    c = bf(tA, tB, M, N, K)
    _, plan = run_exact(s2s, c, with_ws=False)
    assert (plan.launched, plan.bm, plan.bn, plan.reduced, plan.splits[0]) == (1, 64, 64, 0, 1)
    assert plan.nblocks == ((M + 63) // 64) * ((N + 63) // 64)


@pytest.mark.parametrize("tA,tB", gc.FORMS)
@pytest.mark.parametrize("M,N,K,bm,bn", gc.BF16_WIDE_TILES)
def test_wide_tiles_exact(s2s, tA, tB, M, N, K, bm, bn):
    """The 128 x 128 and 64 x 128 instantiations at the smallest shapes that reach them (256 tiles), whole and ragged
    on every edge; the tile is asserted from the launch's record, so a planner change cannot move these to 64 x 64."""
    c = bf(tA, tB, M, N, K)
    _, plan = run_exact(s2s, c)
    assert (plan.launched, plan.bm, plan.bn, plan.reduced, plan.splits[0]) == (1, bm, bn, 0, 1)
    assert plan.nblocks == ((M + bm - 1) // bm) * ((N + bn - 1) // bn) >= 256


@pytest.mark.parametrize("tA,tB", gc.FORMS)
def test_k_zero_empty_and_padded(s2s, tA, tB):
    for opt in gc.K0_OPTIONS:
        c = bf(tA, tB, 40, 33, 0, **opt)
        _, plan = run_exact(s2s, c)
        _assert_plan(plan, [c])
    for M, N, K in gc.EMPTY_SHAPES:
        _, plan = run_exact(s2s, bf(tA, tB, M, N, K, beta=1.0))
        assert plan.launched == 0 and plan.splits[0] == 0
    # Mread / Nread.  BF16_PADDED: K is whole K-tiles of 64 and the tile lies within the declared padding, so the
    # kernel takes the unguarded loads over the caller's zeros, with NaN beyond them; the plain twin takes the
    # guarded ones.  PADDED (K = 96, the fp32 table): the K tail keeps both on the guarded loader, which must ignore
    # the declaration.  Either way the bits are the reference's and the twin's.
    for kw in gc.BF16_PADDED + gc.PADDED:
        c, plain = bf(tA, tB, **kw), bf(tA, tB, **dict(kw, Mread=0, Nread=0))
        if kw in gc.BF16_PADDED:  # the kernel's own fast-path test, for the tile that straddles M / N
            assert c.K % gc.BF16_KTILE == 0 and (c.M % 64 or c.N % 64)
            assert -(-c.M // 64) * 64 <= max(c.M, c.Mread) and -(-c.N // 64) * 64 <= max(c.N, c.Nread)
        out, plan = run_exact(s2s, c, with_ws=False)
        out_plain, _ = run_exact(s2s, plain, with_ws=False)
        assert (plan.bm, plan.bn, plan.splits[0]) == (64, 64, 1)
        assert np.array_equal(gc.bits(c.C.get(out)), gc.bits(plain.C.get(out_plain)))


@pytest.mark.parametrize("tA,tB", gc.FORMS)
def test_direct_epilogue(s2s, tA, tB):
    """bias, rbias, ReLU, alpha and beta one at a time and together in the tile kernel's own epilogue; beta == 0
    over a NaN C window."""
    M, N, K = gc.EPILOGUE_SHAPE
    for opt in gc.EPILOGUES:
        c = bf(tA, tB, M, N, K, **opt)
        if c.beta == 0:
            assert np.isnan(c.C.get()).all()
        _, plan = run_exact(s2s, c, with_ws=False)
        assert (plan.bm, plan.bn, plan.reduced, plan.splits[0]) == (64, 64, 0, 1), opt


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
@pytest.mark.parametrize("M,N,K,s,ks", gc.BF16_SPLIT_SWEEP)
def test_splitk_follows_the_halving_rule(s2s, tA, tB, M, N, K, s, ks):
    """2, 4, 8 and 16 slices, slices of 384 and 448, a ragged last slice: the count and the slice length are the
    library's record of the launch; two runs are bitwise equal."""
    c = bf(tA, tB, M, N, K)
    out, plan = run_exact(s2s, c)
    assert (plan.launched, plan.bm, plan.bn, plan.reduced) == (1, 64, 64, 1)
    assert (plan.splits[0], plan.kslice, plan.nblocks) == (s, ks, s)
    again, plan2 = run_exact(s2s, c)
    assert plan2.splits[0] == s and np.array_equal(gc.bits(out), gc.bits(again))
    _, plan3 = run_exact(s2s, c, with_ws=False)  # no workspace: unsplit, same bits
    assert (plan3.splits[0], plan3.reduced) == (1, 0)


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
@pytest.mark.parametrize("s", gc.SPLIT_EPILOGUE_COUNTS)
@pytest.mark.parametrize("M,N,aligned", gc.SPLIT_EPILOGUE_SHAPES, ids=("f4slab_f4c", "f4slab_scalarc", "scalar"))
def test_splitk_reduce_epilogues(s2s, tA, tB, s, M, N, aligned):
    """Every epilogue flag through the reduce's three paths behind bf16 slabs (K = 768, 2048, 3328: 2 x 384, 8 x 256,
    8 x 448 by the halving rule)."""
    for opt in gc.EPILOGUES:
        c = bf(tA, tB, M, N, 256 * s, aligned=aligned, **opt)
        _, plan = run_exact(s2s, c)
        _, _, ks, splits = _assert_plan(plan, [c])
        assert (splits[0], ks) == {3: (2, 384), 8: (8, 256), 13: (8, 448)}[s] and plan.reduced == 1, opt


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
def test_mixed_batch_alone_and_together(s2s, tA, tB):
    """Two split problems, one unsplit, one with K = 0 and one skipped in one call (K = 1792: 4 slices of 448), then
    each live problem alone under the slice the batch used or its own: the same bits either way."""
    cases = [bf(tA, tB, **kw) for kw in gc.MIXED_BATCH]
    outs, plan = run_batch(s2s, cases)
    _, _, ks, splits = _assert_plan(plan, cases)
    assert (ks, splits) == (448, [4, 4, 1, 1]) and plan.reduced == 1
    for i, (c, out) in enumerate(zip(cases, outs)):
        same_bits(out, c.expect, c.C, f"problem {i} of the batch")
    for c, out in zip(cases[:4], outs[:4]):
        alone, plan1 = run_exact(s2s, c)
        _assert_plan(plan1, [c])
        assert np.array_equal(gc.bits(alone), gc.bits(out))


@pytest.mark.parametrize("tA,tB", gc.SPLIT_FORMS)
def test_sixteen_problems_in_one_call(s2s, tA, tB):
    cases = [bf(tA, tB, **kw) for kw in gc.SIXTEEN]
    outs, plan = run_batch(s2s, cases)
    _assert_plan(plan, cases)
    assert list(plan.splits[:16]) == [1] * 16 and plan.reduced == 0
    for i, (c, out) in enumerate(zip(cases, outs)):
        same_bits(out, c.expect, c.C, f"problem {i} of the batch")


@pytest.mark.parametrize("tA,tB", gc.FORMS)
def test_tile_family_rounds_to_nearest_even(s2s, tA, tB):
    """The rounding leg: operands that are not bf16 numbers, one whole K-tile (unguarded loader) and a K = 40 tail
    (guarded), bitwise the float64 product of the RNE-rounded operands."""
    for kw in gc.BF16_ROUNDING:
        c = bf(tA, tB, data="rounding", **kw)
        _, plan = run_exact(s2s, c, with_ws=False)
        assert (plan.bm, plan.bn, plan.splits[0]) == (64, 64, 1)


@pytest.mark.parametrize("tA,tB,kw", gc.bf16_precision_case_args(),
                         ids=lambda v: f"{v['M']}x{v['N']}x{v['K']}" if isinstance(v, dict) else str(v))
def test_tile_family_precision_on_random_data(s2s, tA, tB, kw):
    c = bf(tA, tB, **kw)
    (out,), plan = run_batch(s2s, [c])
    _assert_plan(plan, [c])
    if c.K == 8192:
        assert plan.splits[0] == 32 and plan.kslice == 256
    if c.M == 2050:
        assert (plan.bm, plan.bn) == (128, 128)
    ratio = np.abs(c.C.get(out).astype(np.float64) - c.ref).max() / np.abs(c.ref).max()
    print(f"bf16 precision ({tA},{tB}) {c.M}x{c.N}x{c.K} splits {plan.splits[0]}: max|gpu-ref|/max|ref| = {ratio:.3e} "
          f"({ratio / gc.PRECISION_BAR:.3f} of the bar)")
    assert np.all(gc.bits(out[c.C.outside()]) == gc.CANARY)
    assert ratio <= gc.PRECISION_BAR, ratio


# ------------------------------------------------------------------------------------------------ the big-tile GEMM
BIG_TILES = ((256, 256), (256, 128), (128, 128))
# (tA, tB, aligned) -> how A and B are staged: K-contiguous operands through stage_kc_bf16 (float4 loads when the
# window is 16-byte aligned with ld % 4 == 0, guarded scalar loads otherwise), the others through stage_rc_bf16
PLACEMENTS = ((0, 1, True, KC_VEC, KC_VEC), (0, 1, False, KC_SCALAR, KC_SCALAR), (1, 0, False, RC, RC),
              (0, 0, True, KC_VEC, RC), (1, 1, False, RC, KC_SCALAR))


@pytest.fixture(scope="module")
def ctx(s2s):
    import s2s_amd
    return s2s_amd.nn.get_context(0)


def big_run(s2s, ctx, c, force=(0, 0, 0)):
    """Case `c` through s2s_debug_gemm_big_run under the override `force` -> (the C array afterwards, the record)."""
    assert c.rbias is None and not c.Mread and not c.Nread
    a, b, cd = dev(c.A.buf), dev(c.B.buf), dev(c.C.buf)
    bd = dev(c.bias.buf) if c.bias is not None else None
    done, rec = ctypes.c_int(0), s2s.BigPlan()
    assert s2s.lib.s2s_debug_gemm_big_force(*force) == 0
    try:
        rc = s2s.lib.s2s_debug_gemm_big_run(ctx.handle, stream(), c.tA, c.tB, c.M, c.N, c.K, c.alpha, ptr(a, c.A.off),
                                            c.A.ld, ptr(b, c.B.off), c.B.ld, c.beta, ptr(cd, c.C.off), c.C.ld,
                                            ptr(bd, c.bias.off) if bd is not None else None, c.relu, ctypes.byref(done))
        s2s.lib.s2s_debug_gemm_big_last(ctypes.byref(rec))
    finally:
        assert s2s.lib.s2s_debug_gemm_big_force(0, 0, 0) == 0
    ok(s2s, rc)
    torch.cuda.synchronize()
    assert done.value == 1 and (rec.launched, rec.declined) == (1, 0)
    return cd.cpu().numpy(), rec


def big_exact(s2s, ctx, c, force=(0, 0, 0)):
    out, rec = big_run(s2s, ctx, c, force)
    same_bits(out, c.expect, c.C, f"big {(c.tA, c.tB, c.M, c.N, c.K)} force {force} alpha {c.alpha} beta {c.beta}")
    return out, rec


def _big_shapes(bm, bn):
    return ((bm, bn, 64), (bm + 13, bn + 5, 133), (bm, bn, 320))


@pytest.mark.parametrize("bm,bn", BIG_TILES)
@pytest.mark.parametrize("which", (0, 1, 2), ids=("whole", "ragged", "k320"))
def test_big_every_tile_and_staging_path(s2s, ctx, bm, bn, which):
    """Each of the three tiles, forced at a small shape: one whole tile at K = 64, a second ragged tile each way with
    K % 8 != 0 and K % 64 != 0, and K = 320 (five K-tiles through both LDS stages), in every placement: both paths of
    stage_kc_bf16 and stage_rc_bf16, asserted from the record."""
    M, N, K = _big_shapes(bm, bn)[which]
    for tA, tB, aligned, sa, sb in PLACEMENTS:
        c = bf(tA, tB, M, N, K, aligned=aligned, alpha=1.0, beta=0.0)
        _, rec = big_exact(s2s, ctx, c, (bm, bn, 1))
        tiles = ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
        assert (rec.bm, rec.bn, rec.S, rec.kslice, rec.nblocks, rec.forced) == (bm, bn, 1, (K + 63) // 64, tiles, 1)
        assert (rec.stage_a, rec.stage_b) == (sa, sb), (tA, tB, aligned)


@pytest.mark.parametrize("S", (2, 3, 4, 16, 17, 33))
def test_big_slab_sums(s2s, ctx, S):
    """bf16_splitk_reduce over S slabs of two K-tiles, the last of one and ragged in K (K = 64 (2 S - 1) - 27): the
    16-wide loop alone (16), its tail alone (2, 3, 4), and both (17, 33); two runs are bitwise equal."""
    K = 64 * (2 * S - 1) - 27
    for (tA, tB, aligned, sa, sb), (bm, bn) in zip(PLACEMENTS[:3], BIG_TILES[::-1]):
        c = bf(tA, tB, 141, 133, K, aligned=aligned)
        out, rec = big_exact(s2s, ctx, c, (bm, bn, S))
        tiles = ((141 + bm - 1) // bm) * ((133 + bn - 1) // bn)
        assert (rec.bm, rec.bn, rec.S, rec.kslice, rec.nblocks) == (bm, bn, S, 2, tiles * S)
        assert (rec.stage_a, rec.stage_b) == (sa, sb)
        again, _ = big_exact(s2s, ctx, c, (bm, bn, S))
        assert np.array_equal(gc.bits(out), gc.bits(again))


BIG_EPILOGUES = tuple(o for o in gc.EPILOGUES if not o.get("rbias")) + (
    gc._k(alpha=-2.0, beta=0.25, bias=True, relu=True), gc._k(alpha=0.5, beta=1.0, bias=True, relu=True),
    gc._k(alpha=1.0, beta=0.0, bias=True, relu=True))


@pytest.mark.parametrize("S", (1, 3), ids=("unsplit", "split"))
@pytest.mark.parametrize("tA,tB,aligned", ((0, 1, True), (1, 0, False)))
def test_big_epilogues(s2s, ctx, S, tA, tB, aligned):
    """bias, beta in {0, 0.25, 1}, ReLU and alpha one at a time and together, in the tile kernel's epilogue (S = 1)
    and in the reduce's (S = 3); beta == 0 over a NaN C window."""
    betas = set()
    for opt in BIG_EPILOGUES:
        c = bf(tA, tB, 141, 133, 315, aligned=aligned, **opt)
        betas.add(c.beta)
        _, rec = big_exact(s2s, ctx, c, (128, 128, S))
        assert (rec.S, rec.kslice) == (S, 5 if S == 1 else 2), opt
    assert {0.0, 0.25, 1.0} <= betas


def test_big_time_model_is_pinned(s2s, ctx):
    """Without the override, one shape per tile: what the time model picks today, from the record.  (2000, 4096, 96):
    256 x 128 in one wave of 256 workgroups beats 128 tiles of 256 x 256 on half the chip.)"""
    for (M, N, K), want in (((2100, 4096, 64), (256, 256, 1, 1, 144)), ((4096, 2048, 64), (256, 128, 1, 1, 256)),
                            ((2000, 4096, 96), (256, 128, 1, 2, 256)), ((1000, 2000, 64), (128, 128, 1, 1, 128)),
                            ((300, 200, 1030), (128, 128, 4, 5, 24))):
        c = bf(0, 1, M, N, K, aligned=True, alpha=1.0, beta=0.0)
        _, rec = big_exact(s2s, ctx, c)
        assert (rec.bm, rec.bn, rec.S, rec.kslice, rec.nblocks) == want and rec.forced == 0, (M, N, K)


def test_big_declines_what_it_cannot_run(s2s, ctx):
    """rbias, Mread and Nread: done == 0, the record says declined, and C is bitwise untouched."""
    for kw in (gc._k(rbias=True), gc._k(Mread=192), gc._k(Nread=192)):
        c = bf(0, 1, 141, 133, 133, alpha=1.0, beta=0.0, **kw)
        probs, keep = (s2s.Problem * 1)(), []
        cd = fill_problem(probs[0], c, keep)
        done, rec = ctypes.c_int(1), s2s.BigPlan()
        ok(s2s, s2s.lib.s2s_debug_gemm_big_problem(ctx.handle, stream(), probs, c.tA, c.tB, ctypes.byref(done)))
        s2s.lib.s2s_debug_gemm_big_last(ctypes.byref(rec))
        torch.cuda.synchronize()
        assert done.value == 0 and (rec.launched, rec.declined) == (0, 1), kw
        same_bits(cd.cpu().numpy(), c.C.buf, c.C, f"declined {kw}")
    # the same entry runs a plain problem
    c = bf(0, 1, 141, 133, 133, alpha=1.0, beta=0.0)
    probs, keep = (s2s.Problem * 1)(), []
    cd = fill_problem(probs[0], c, keep)
    done = ctypes.c_int(0)
    ok(s2s, s2s.lib.s2s_debug_gemm_big_problem(ctx.handle, stream(), probs, c.tA, c.tB, ctypes.byref(done)))
    torch.cuda.synchronize()
    assert done.value == 1
    same_bits(cd.cpu().numpy(), c.expect, c.C, "big_problem")


@pytest.mark.parametrize("K", (133, 315))
def test_big_override_refuses_a_split_it_cannot_run(s2s, ctx, K):
    """K = 133 has three K-tiles, fewer than a forced split of 4; K = 315 has five, which cut into slices of two
    K-tiles make 3 slices, not 4: either call fails on the host, launches nothing and leaves C alone."""
    c = bf(0, 1, 141, 133, K, alpha=1.0, beta=0.0)
    a, b, cd = dev(c.A.buf), dev(c.B.buf), dev(c.C.buf)
    done = ctypes.c_int(1)
    assert s2s.lib.s2s_debug_gemm_big_force(128, 128, 4) == 0
    try:
        rc = s2s.lib.s2s_debug_gemm_big_run(ctx.handle, stream(), 0, 1, c.M, c.N, c.K, 1.0, ptr(a, c.A.off), c.A.ld,
                                            ptr(b, c.B.off), c.B.ld, 0.0, ptr(cd, c.C.off), c.C.ld, None, 0,
                                            ctypes.byref(done))
    finally:
        assert s2s.lib.s2s_debug_gemm_big_force(0, 0, 0) == 0
    torch.cuda.synchronize()
    assert rc != 0 and done.value == 0 and "forced split" in s2s.lib.s2s_last_error().decode()
    same_bits(cd.cpu().numpy(), c.C.buf, c.C, "refused override")


@pytest.mark.parametrize("bm,bn", BIG_TILES)
def test_big_rounds_to_nearest_even(s2s, ctx, bm, bn):
    """The rounding leg through both staging kernels (and both paths of stage_kc_bf16): K = 64, and K = 40 through
    the guarded loads and the zero padding of the K-tile."""
    for K in (64, 40):
        for tA, tB, aligned, sa, sb in PLACEMENTS[:3]:
            c = bf(tA, tB, 77, 45, K, aligned=aligned, data="rounding", bias=True, beta=0.25)
            _, rec = big_exact(s2s, ctx, c, (bm, bn, 1))
            assert (rec.bm, rec.bn, rec.stage_a, rec.stage_b) == (bm, bn, sa, sb)


@pytest.mark.parametrize("M,N,K,force", ((269, 261, 133, (256, 256, 1)), (141, 133, 1030, (128, 128, 4))),
                         ids=("unsplit", "split"))
def test_big_precision_on_random_data(s2s, ctx, M, N, K, force):
    c = bf(1, 0, M, N, K, **gc.PRECISION_OPTIONS)
    out, rec = big_run(s2s, ctx, c, force)
    assert (rec.bm, rec.bn, rec.S) == force
    ratio = np.abs(c.C.get(out).astype(np.float64) - c.ref).max() / np.abs(c.ref).max()
    print(f"big bf16 precision {M}x{N}x{K} {force}: max|gpu-ref|/max|ref| = {ratio:.3e}")
    assert np.all(gc.bits(out[c.C.outside()]) == gc.CANARY)
    assert ratio <= gc.PRECISION_BAR, ratio


# ------------------------------------------------------------------------------------------------ the convolutions
def _ints(rng, shape):
    return gc.draw(rng, shape, True)


def _rvals(rng, shape):
    return gc.draw(rng, shape, "rounding")


def _f32_exact(ref, what):
    """float64 reference -> its fp32 bits, asserting that it is an fp32 number (the bound of the data used)."""
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref), f"{what}: the reference is not an fp32 number"
    return r32


def _conv_case(rng, B, Cin, H, W, Cout, k, draw_op):
    x = draw_op(rng, (B, Cin, H, W))
    Wt = draw_op(rng, (Cout, Cin * k * k))
    bias = _ints(rng, (Cout,))
    dy = draw_op(rng, (B, Cout, H - k + 1, W - k + 1))
    gw0 = _ints(rng, (Cout, Cin * k * k))
    return x, Wt, bias, dy, gw0


def _conv_reference(x, Wt, bias, dy, gw0, k, relu, scale):
    """float64 convolution of the RNE-rounded operands: y, dx, dW (onto gw0), db."""
    B, Cin = x.shape[:2]
    Cout = Wt.shape[0]
    xr = gc.bf16_round(x).astype(np.float64)
    Wr = gc.bf16_round(Wt).astype(np.float64).reshape(Cout, Cin, k, k)
    xw = win(xr, (k, k), axis=(2, 3))
    pre = np.einsum("bchwij,ocij->bohw", xw, Wr, optimize=True) + bias.astype(np.float64)[None, :, None, None]
    y = np.maximum(pre, 0.0) if relu else pre
    dyt = dy.astype(np.float64) * (pre > 0) if relu else dy.astype(np.float64)
    dyr = gc.bf16_round(dyt.astype(np.float32)).astype(np.float64)
    pad = np.pad(dyr, ((0, 0), (0, 0), (k - 1, k - 1), (k - 1, k - 1)))
    dx = np.einsum("bohwij,ocij->bchw", win(pad, (k, k), axis=(2, 3)), Wr[:, :, ::-1, ::-1], optimize=True)
    dW = gw0 + scale * np.einsum("bohw,bchwij->ocij", dyr, xw, optimize=True).reshape(Cout, Cin * k * k)
    db = scale * dyt.sum(axis=(0, 2, 3))
    return y, dx + 0.0, dW, db + 0.0


def _conv_run(s2s, B, Cin, H, W, Cout, k, relu, prec, implicit, data, scale=0.5, check_db=True):
    import s2s_amd
    from s2s_amd import frontend as fe
    from s2s_amd import profile as prof
    knob = s2s.lib.s2s_debug_sconv_wgrad_implicit
    knob.argtypes = [ctypes.c_int]
    rng = np.random.default_rng(B * 1000 + Cin + 7 * H + k)
    x, Wt, bias, dy, gw0 = data(rng)
    conv = fe.SpatialConvolutionMM(Cin, Cout, k, k, relu=relu)
    conv.weight, conv.bias = torch.tensor(Wt, device="cuda"), torch.tensor(bias, device="cuda")
    conv.gradWeight, conv.gradBias = torch.tensor(gw0, device="cuda"), torch.zeros(Cout, device="cuda")
    xg, dyg = torch.tensor(x, device="cuda"), torch.tensor(dy, device="cuda")
    knob(implicit)
    s2s.lib.s2s_prof_enable(1)
    try:
        prof.collect()
        with s2s_amd.precision(prec):
            y = conv.forward(xg).clone()
            dx = conv.backward(xg, dyg, scale).clone()
        torch.cuda.synchronize()
        ran = prof.collect()
    finally:
        s2s.lib.s2s_prof_enable(0)
        knob(1)
    yr, dxr, dWr, dbr = _conv_reference(x, Wt, bias, dy, gw0, k, relu, scale)
    what = f"conv {(B, Cin, H, W, Cout, k)} relu {relu} {prec} implicit {implicit}"
    same_bits(y.cpu().numpy().ravel(), _f32_exact(yr, "y").ravel(), None, what + " y")
    same_bits(dx.cpu().numpy().ravel(), _f32_exact(dxr, "dx").ravel(), None, what + " dx")
    same_bits(conv.gradWeight.cpu().numpy().ravel(), _f32_exact(dWr, "dW").ravel(), None, what + " dW")
    if check_db:  # (a plain fp32 column sum of dy, no bf16 kernel: exact on integer data only)
        same_bits(conv.gradBias.cpu().numpy().ravel(), _f32_exact(dbr, "db").ravel(), None, what + " db")
    return ran


CONV_SHAPES = ((2, 3, 20, 12, 64, 3, True),     # the first layer's form: K = 27, W read as it is
               (2, 64, 17, 11, 64, 3, False),   # tap-major K over the channels-last copy, K = 576
               (1, 128, 9, 13, 128, 3, True),   # two channel tiles each way
               (3, 5, 7, 6, 7, 3, False),       # every edge ragged, K = 45
               (2, 64, 6, 5, 64, 1, True))      # a 1 x 1 kernel: one tap, K = 64


@pytest.mark.parametrize("prec,implicit", (("bf16", 1), ("bf16-all", 1), ("bf16-all", 0)))
@pytest.mark.parametrize("B,Cin,H,W,Cout,k,relu", CONV_SHAPES)
def test_implicit_convolutions_exact(s2s, B, Cin, H, W, Cout, k, relu, prec, implicit):
    """SpatialConvolutionMM under bf16 / bf16-all on integer x, W, bias, dy and a non-zero integer gradWeight start
    with scale 0.5: y, dx, dW and db are bitwise the float64 convolution (the pre-activations agree exactly, so the
    ReLU mask is no judgement call).  The profile proves the implicit kernels ran; under bf16-all the weight gradient
    takes conv_wgrad_bf16_kernel for Cin % 64 == 0 unless the knob forces the im2col panel."""
    ran = _conv_run(s2s, B, Cin, H, W, Cout, k, relu, prec, implicit,
                    lambda rng: _conv_case(rng, B, Cin, H, W, Cout, k, _ints))
    assert "conv_fwd_bf16" in ran and "conv_dx_bf16" in ran, sorted(ran)
    assert ("conv_wgrad_bf16" in ran) == (prec == "bf16-all" and implicit == 1 and Cin % 64 == 0), sorted(ran)


@pytest.mark.parametrize("B,Cin,H,W,Cout,k", ((3, 5, 7, 6, 7, 3), (1, 64, 6, 8, 64, 1), (2, 3, 6, 7, 7, 3)))
def test_convolutions_round_to_nearest_even(s2s, B, Cin, H, W, Cout, k):
    """The rounding leg: x, W and dy that are not bf16 numbers, every reduction at most 64 long (Cin k k, Cout k k and
    B Ho Wo), so y, dx and dW are bitwise the float64 convolution of the RNE-rounded operands."""
    assert Cin * k * k <= 64 and Cout * k * k <= 64 and B * (H - k + 1) * (W - k + 1) <= 64
    ran = _conv_run(s2s, B, Cin, H, W, Cout, k, False, "bf16-all", 1,
                    lambda rng: _conv_case(rng, B, Cin, H, W, Cout, k, _rvals), check_db=False)
    assert "conv_fwd_bf16" in ran and "conv_dx_bf16" in ran and ("conv_wgrad_bf16" in ran) == (Cin % 64 == 0)


# ------------------------------------------------------------------------------------------------ the linear layer
@pytest.mark.parametrize("big", (1, 0))
@pytest.mark.parametrize("B,L,Din,Dout,relu,data", ((2, 50, 64, 40, True, "exact"), (2, 512, 1024, 512, True, "exact"),
                                                     (1, 60, 64, 40, False, "rounding")))
def test_linear_layer_exact(s2s, big, B, L, Din, Dout, relu, data):
    """TemporalConvolution(Din, Dout, 1) under bf16-all on exact data: forward, input gradient, weight and bias
    gradients bitwise the float64 products -- on the big-tile GEMM where all three products are large (asserted from
    its call counter), on the tile family otherwise or when big = 0; and the rounding leg (B L, Din, Dout <= 64)."""
    import s2s_amd
    from s2s_amd import frontend as fe
    knob, calls = s2s.lib.s2s_debug_gemm_big, s2s.lib.s2s_debug_gemm_big_calls
    knob.argtypes, calls.restype = [ctypes.c_int], ctypes.c_long
    rng = np.random.default_rng(B + L + Din)
    op = _ints if data == "exact" else _rvals
    x, W, dy = op(rng, (B, L, Din)), op(rng, (Dout, Din)), op(rng, (B, L, Dout))
    b = _ints(rng, (Dout,))
    m = fe.TemporalConvolution(Din, Dout, 1, relu=relu)
    m.weight, m.bias = torch.tensor(W, device="cuda"), torch.tensor(b, device="cuda")
    m.gradWeight, m.gradBias = torch.zeros_like(m.weight), torch.zeros_like(m.bias)
    xg, dyg = torch.tensor(x, device="cuda"), torch.tensor(dy, device="cuda")
    n0 = calls()
    knob(big)
    try:
        with s2s_amd.precision("bf16-all"):
            y = m.forward(xg).clone()
            dx = m.backward(xg, dyg, 0.5).clone()
        torch.cuda.synchronize()
    finally:
        knob(1)
    large = 2.0 * B * L * Din * Dout >= 1e9
    assert calls() - n0 == (3 if big and large else 0)
    xr = gc.bf16_round(x).astype(np.float64).reshape(B * L, Din)
    Wr = gc.bf16_round(W).astype(np.float64)
    pre = xr @ Wr.T + b.astype(np.float64)
    dyt = dy.reshape(B * L, Dout).astype(np.float64) * ((pre > 0) if relu else 1.0)
    dyr = gc.bf16_round(dyt.astype(np.float32)).astype(np.float64)
    what = f"linear {(B, L, Din, Dout)} big {big} "
    same_bits(y.cpu().numpy().ravel(), _f32_exact(np.maximum(pre, 0) if relu else pre, "y").ravel(), None, what + "y")
    same_bits(dx.cpu().numpy().ravel(), _f32_exact(dyr @ Wr + 0.0, "dx").ravel(), None, what + "dx")
    same_bits(m.gradWeight.cpu().numpy().ravel(), _f32_exact(0.5 * dyr.T @ xr + 0.0, "dW").ravel(), None, what + "dW")
    if data == "exact":  # (a plain fp32 column sum of dy, no bf16 kernel: exact on integer data only)
        same_bits(m.gradBias.cpu().numpy().ravel(), _f32_exact(0.5 * dyt.sum(0) + 0.0, "db").ravel(), None, what + "db")
