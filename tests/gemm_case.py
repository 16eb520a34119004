"""Cases for the direct tests of the fp32 GEMM family (csrc/gemm_f32.hip), in plain numpy: no GPU is imported here, so
the CPU suite can check the cases themselves (tests/test_gemm_case_cpu.py) and the GPU suite runs them
(tests/test_gpu_gemm_f32.py).

Placement.  Every operand and every output of a case is a window inside a larger 1-D float32 array (`Win`): the
window starts at an odd float offset (a 4-byte-aligned address, no more) and its leading dimension is odd and larger
than the window, unless the case asks for `aligned` (16-byte-aligned start, ld % 4 == 0: what the float4 epilogue of
the split-K reduce needs).  Input arrays are NaN outside their window, so a read outside it that reaches an
accumulator turns up as NaN in C; output arrays hold CANARY outside their window and must come back bitwise unchanged.
Where a case sets Mread / Nread, the window of that operand is widened to the declared padding, which is zeros;
beyond it is NaN again.

Exact data (the default): A, B, C0, bias and rbias are non-zero integers in -4..-1, 1..4 and alpha, beta come from
{1, 0.5, 0.25, -2, 0}.  Every product is an integer of magnitude <= 16, so with K <= 6144 every partial sum of any
subset of terms, in any order, is an integer below 2^17 and the whole expression a multiple of 1/4 below 2^19: fp32
represents all of them, no operation rounds, and the float64 reference is the one answer an fp32 kernel can give.
The comparison is then bitwise.  Because no value is zero, a dropped, doubled or misplaced term changes the result.
(Signed zeros: an accumulator that cancels is +0 in either precision, and alpha * (+0) = -0 for alpha < 0 in both; only
max(-0, +0) is left open by IEEE 754, so a ReLU case must add something non-zero after the product whenever
alpha <= 0 -- `build_case` refuses the others.)

Random data (the precision leg only): A, B, C0 and bias standard normal, compared against the float64 reference at
PRECISION_BAR.

bf16 kernels (precision="bf16": gemm_bf16_kernel, the big-tile GEMM of csrc/gemm_bf16.hip) round A and B to bf16 with
round-to-nearest-even before they multiply and accumulate in fp32.  The integers -4..4 are bf16 numbers, so the exact
data is untouched by that rounding (build_case asserts it) and the same bitwise comparison holds.  The rounding leg
(data="rounding") puts values in A and B that are not bf16 numbers but whose roundings are small dyadic ones: still
bitwise, and the expected bits differ under truncation, ties-away and no rounding (tests/test_gemm_case_cpu.py).
The reference of a bf16 case is always the float64 product of the RNE-rounded operands.

Reference: alpha * op(A) op(B) + bias[col] + rbias[row] + beta * C0, then ReLU, in float64.  beta == 0 means C0 is not
read: the C window then holds NaN, which must not appear in the result.
"""
import zlib

import numpy as np

CANARY = np.uint32(0xCAFEF00D)  # -8353798.5 as a float: not a value any case produces
SCALARS = (1.0, 0.5, 0.25, -2.0, 0.0)
PRECISION_BAR = 2e-5  # max|gpu - ref| <= PRECISION_BAR * max|ref| (the bar of tests/test_gpu_bf16.py)
KMAX_EXACT = 6144


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canary_f32():
    return np.array([CANARY], dtype=np.uint32).view(np.float32)[0]


class Win:
    """A rows x cols window at float offset `off` with leading dimension `ld` inside the 1-D float32 array `buf`."""

    def __init__(self, rows, cols, fill, aligned=False):
        self.rows, self.cols = int(rows), int(cols)
        if aligned:
            self.off, self.ld = 8, (self.cols + 4 + 3) // 4 * 4
        else:
            self.off, self.ld = 5, (self.cols + 6) | 1
        assert self.ld > self.cols
        assert (self.off % 4 == 0 and self.ld % 4 == 0) if aligned else (self.off % 2 == 1 and self.ld % 2 == 1)
        self.buf = np.full(self.off + max(self.rows, 1) * self.ld + 9, fill, dtype=np.float32)

    def index(self):
        return self.off + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]

    def get(self, buf=None):
        return (self.buf if buf is None else buf)[self.index()]

    def put(self, values):
        self.buf[self.index()] = np.asarray(values, dtype=np.float32).reshape(self.rows, self.cols)
        return self

    def outside(self):
        m = np.ones(self.buf.size, dtype=bool)
        m[self.index().ravel()] = False
        return m


def draw(rng, shape, exact):
    """float32 test data: non-zero integers in -4..-1, 1..4 (exact), standard normal, or (exact == "rounding") the
    values of ROUNDING_VALUES."""
    if isinstance(exact, str) and exact == "rounding":
        return rng.choice(ROUNDING_VALUES, size=shape).astype(np.float32)
    if exact:
        return (rng.integers(1, 5, size=shape) * rng.choice((-1, 1), size=shape)).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


# The rounding leg (bf16 only): fp32 values that are NOT bf16 numbers, whose RNE roundings are multiples of 2^-7 of
# magnitude <= 4 -- ties that go down to even and up to even, just above and just below a tie, and the carry into
# the exponent -- times +-1, +-2.  Products of the rounded values are multiples of 2^-14 of magnitude <= 16, so with
# K <= KMAX_ROUNDING every partial sum, in any order, is a multiple of 2^-14 of magnitude <= 2^10: 24 bits, exact in
# fp32, and alpha in {1, -2} only moves the exponent.
_E = 2.0 ** -23
ROUNDING_PATTERNS = (1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8,                          # ties: down to even, up to even
                     1 + 2.0 ** -8 + _E, 1 + 2.0 ** -8 - _E,                            # just above / below a tie
                     1 + 2.0 ** -7 + 2.0 ** -8 + _E, 1 + 2.0 ** -7 + 2.0 ** -8 - _E,
                     1.5 + 2.0 ** -8, 1.75 + 2.0 ** -7 + 2.0 ** -8,                     # ties at other mantissas
                     2 - 2.0 ** -9, 2 - 2.0 ** -8)                                      # the carry into the exponent
ROUNDING_VALUES = np.array([f * p for p in ROUNDING_PATTERNS for f in (1, -1, 2, -2)], dtype=np.float32)
assert np.array_equal(ROUNDING_VALUES.astype(np.float64),
                      np.array([f * p for p in ROUNDING_PATTERNS for f in (1, -1, 2, -2)]))  # all are fp32 numbers
KMAX_ROUNDING = 64
ROUNDING_ALPHAS = (1.0, -2.0)


class Case:
    pass


def build_case(tA, tB, M, N, K, alpha=None, beta=None, bias=False, rbias=False, relu=False, Mread=0, Nread=0,
               aligned=False, data="exact", seed=0, precision="f32"):
    """One GEMM problem: windows A, B, C (and bias, rbias or None), the float64 reference `ref` (M x N), and
    `expect`: the whole C array as it must read afterwards (canary, and for exact data the result in fp32).
    alpha / beta left None are drawn (alpha from the non-zero SCALARS: a product scaled by 0 checks nothing; the
    epilogue tables give alpha = 0 explicitly).  The draws do not depend on Mread / Nread / aligned, so the same
    arguments with and without them give the same problem.
    precision: "f32", or "bf16" for kernels that round A and B to bf16 (RNE) before they multiply: the reference is
    then the float64 product of the rounded operands (`mulA`, `mulB`); bias, rbias and C0 are never rounded.  Exact
    data must then be bf16 numbers already (asserted).  data = "rounding" (bf16 only): the values of ROUNDING_VALUES
    in A and B, integers elsewhere; the comparison is bitwise like the exact one, under the bound asserted here."""
    rounding = data == "rounding"
    exact = data == "exact"
    assert data in ("exact", "random", "rounding") and precision in ("f32", "bf16")
    assert not exact or K <= KMAX_EXACT
    assert not rounding or (precision == "bf16" and K <= KMAX_ROUNDING)
    rng = np.random.default_rng(zlib.crc32(repr((tA, tB, M, N, K, seed, data)).encode()))
    a = draw(rng, (M, K), "rounding" if rounding else exact)
    b = draw(rng, (K, N), "rounding" if rounding else exact)
    exact = exact or rounding  # everything else about a rounding case is an exact case
    c0 = draw(rng, (M, N), exact)
    bv = draw(rng, (N,), exact)
    rv = draw(rng, (M,), True)
    da, db = rng.choice(SCALARS[:4]), rng.choice(SCALARS)
    if rounding and alpha is None:
        da = ROUNDING_ALPHAS[int(rng.integers(0, 2))]
    alpha = float(da if alpha is None else alpha)
    beta = float(db if beta is None else beta)
    assert not rounding or alpha in ROUNDING_ALPHAS
    assert not (exact and relu and alpha <= 0 and not bias and not rbias and beta == 0), "max(-0, +0) is not pinned"

    c = Case()
    c.tA, c.tB, c.M, c.N, c.K = int(tA), int(tB), M, N, K
    c.alpha, c.beta, c.relu, c.Mread, c.Nread, c.exact = alpha, beta, int(relu), Mread, Nread, exact
    c.precision, c.data = precision, data
    nan = np.float32(np.nan)
    Mr, Nr = max(M, Mread), max(N, Nread)
    ap = np.zeros((Mr, K), np.float32)
    ap[:M] = a
    bp = np.zeros((K, Nr), np.float32)
    bp[:, :N] = b
    c.A = Win(K, Mr, nan, aligned).put(ap.T) if tA else Win(Mr, K, nan, aligned).put(ap)
    c.B = Win(Nr, K, nan, aligned).put(bp.T) if tB else Win(K, Nr, nan, aligned).put(bp)
    c.C = Win(M, N, canary_f32(), aligned).put(c0 if beta != 0 else np.full((M, N), nan))
    c.bias = Win(1, N, nan, aligned).put(bv) if bias else None
    c.rbias = Win(1, M, nan, aligned).put(rv) if rbias else None
    c.opA, c.opB, c.C0 = a, b, c0
    c.mulA, c.mulB = (bf16_round(a), bf16_round(b)) if precision == "bf16" else (a, b)
    if precision == "bf16" and data == "exact":  # exact data survives the kernels' rounding unchanged
        assert np.array_equal(bits(c.mulA), bits(a)) and np.array_equal(bits(c.mulB), bits(b))
    c.biasv, c.rbiasv = (bv if bias else None), (rv if rbias else None)
    c.ref = reference(c, np.float64)
    if rounding:
        # the bound: rounded operands are multiples of 2^-7 of magnitude <= 4, so any partial sum of <= 64 products
        # is a multiple of 2^-14 of magnitude <= 2^10 (24 bits); every rounded value differs from its operand
        for m, o in ((c.mulA, a), (c.mulB, b)):
            assert np.array_equal(m * 128, np.round(m * 128)) and np.abs(m).max(initial=0) <= 4 and np.all(m != o)
        assert (np.abs(c.mulA.astype(np.float64)) @ np.abs(c.mulB.astype(np.float64))).max(initial=0) <= 2.0 ** 10
        assert np.array_equal(c.ref.astype(np.float32).astype(np.float64), c.ref)  # with this case's epilogue too
    c.expect = c.C.buf.copy()
    if exact:
        c.expect[c.C.index()] = c.ref.astype(np.float32)
    return c


def reference(c, dtype, kslice=0, opA=None, opB=None):
    """The case's expression evaluated in `dtype`, in the kernels' epilogue order; kslice > 0 sums the product in
    slices along K (as split-K does), each slice computed on its own."""
    a = (c.mulA if opA is None else opA).astype(dtype)
    b = (c.mulB if opB is None else opB).astype(dtype)
    if kslice > 0 and c.K > 0:
        prod = np.zeros((c.M, c.N), dtype)
        for k0 in range(0, c.K, kslice):
            prod = prod + a[:, k0:k0 + kslice] @ b[k0:k0 + kslice]
    else:
        prod = a @ b
    v = dtype(c.alpha) * prod
    if c.biasv is not None:
        v = v + c.biasv.astype(dtype)[None, :]
    if c.rbiasv is not None:
        v = v + c.rbiasv.astype(dtype)[:, None]
    if c.beta != 0:
        v = v + dtype(c.beta) * c.C0.astype(dtype)
    if c.relu:
        v = np.maximum(v, dtype(0))
    assert v.dtype == dtype
    return v


def declare(lib):
    """ctypes signatures of the test entry points of csrc/capi_debug.cpp (s2s_debug_gemm_batch and the helpers' entries);
    -> a namespace with the argument structs Problem, Plan and ColsumOut."""
    import ctypes as ct
    vp, i, f, lg, sz = ct.c_void_p, ct.c_int, ct.c_float, ct.c_long, ct.c_size_t

    class Problem(ct.Structure):  # s2s_debug_gemm_problem
        _fields_ = [("A", vp), ("B", vp), ("C", vp), ("bias", vp), ("rbias", vp), ("lda", lg), ("ldb", lg), ("ldc", lg),
                    ("M", i), ("N", i), ("K", i), ("alpha", f), ("beta", f), ("Mread", i), ("Nread", i), ("relu", i)]

    class Plan(ct.Structure):  # s2s_debug_gemm_plan
        _fields_ = [("launched", i), ("bm", i), ("bn", i), ("kslice", i), ("nblocks", i), ("reduced", i),
                    ("splits", i * 16)]

    class BigPlan(ct.Structure):  # s2s_debug_gemm_big_plan
        _fields_ = [(n, i) for n in ("launched", "declined", "bm", "bn", "S", "kslice", "nblocks", "stage_a",
                                     "stage_b", "forced")]

    class ColsumOut(ct.Structure):  # s2s_debug_colsum_out
        _fields_ = [("col0", i), ("ncols", i), ("dst", vp * 3), ("ndst", i)]

    sigs = {
        "s2s_debug_gemm": [i, i, i, i, i, f, vp, lg, vp, lg, f, vp, lg, i, vp, sz],
        "s2s_debug_gemm_batch": [vp, ct.POINTER(Problem), i, i, i, vp, sz, ct.POINTER(Plan)],
        "s2s_debug_gemm_batch_prec": [vp, ct.POINTER(Problem), i, i, i, i, vp, sz, ct.POINTER(Plan)],
        "s2s_debug_gemm_big_run": [vp, vp, i, i, i, i, i, f, vp, lg, vp, lg, f, vp, lg, vp, i, ct.POINTER(i)],
        "s2s_debug_gemm_big_problem": [vp, vp, ct.POINTER(Problem), i, i, ct.POINTER(i)],
        "s2s_debug_gemm_big_force": [i, i, i],
        "s2s_debug_colsum": [vp, vp, lg, i, i, f, f, vp, vp, sz],
        "s2s_debug_colsum_scatter": [vp, vp, lg, i, i, f, ct.POINTER(ColsumOut), i, vp, sz],
        "s2s_debug_copy2d": [vp, vp, lg, vp, lg, i, i, i],
        "s2s_debug_transpose": [vp, vp, lg, i, i, vp, lg],
        "s2s_debug_pad_cols": [vp, vp, lg, vp, i, i, i],
        "s2s_debug_axpby": [vp, vp, vp, sz, f, f],
        "s2s_debug_fill_u32": [vp, vp, ct.c_uint, sz],
        "s2s_debug_zero": [vp, vp, sz],
    }
    for name, argtypes in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = i, argtypes
    lib.s2s_debug_gemm_big_last.restype, lib.s2s_debug_gemm_big_last.argtypes = None, [ct.POINTER(BigPlan)]
    lib.s2s_last_error.restype = ct.c_char_p

    class E:
        pass

    E.Problem, E.Plan, E.ColsumOut, E.BigPlan = Problem, Plan, ColsumOut, BigPlan
    return E


def bf16_round(a):
    """float32 -> nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def bf16_truncate(a):
    """float32 -> bf16 by dropping the low 16 bits (round toward zero), as float32: NOT what the kernels do."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_round_ties_away(a):
    """float32 -> nearest bf16 with ties away from zero, as float32: NOT what the kernels do."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x8000) >> 16) << 16).astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------ the case tables
# Each entry is the keyword set of build_case; the GPU tests run every one, the CPU tests check every one.
FORMS = ((0, 0), (0, 1), (1, 0), (1, 1))
SPLIT_FORMS = ((0, 0), (1, 0))  # (0, 0) is the weight-gradient form


def _k(**kw):
    return kw


SINGLE_SHAPES = (
    (64, 64, 32),                     # one whole tile, one whole K-tile: unguarded loads only
    (64, 64, 369), (64, 128, 100),    # fast tiles whose last K-tile takes the guarded loader
    (77, 45, 133),                    # every edge ragged
    (129, 64, 64), (64, 65, 64),      # a second tile of one row / one column
    (192, 192, 64), (64 * 17, 64, 32),  # 9 and 17 blocks: grid rounded up to 8, XCD remap
    (5, 3, 1), (33, 7, 3), (64, 64, 31),  # K below one K-tile
)
K0_OPTIONS = tuple(_k(bias=b, beta=be, alpha=al) for b in (False, True) for be, al in ((0.0, 1.0), (0.25, -2.0)))
EMPTY_SHAPES = ((0, 5, 64), (5, 0, 64))
PADDED = (_k(M=64, N=40, K=96, Nread=64), _k(M=40, N=64, K=96, Mread=64))
# one flag at a time, then together (alpha = 0 last: C = bias + beta C whatever the product)
EPILOGUES = (
    _k(alpha=1.0, beta=0.0, bias=True),
    _k(alpha=1.0, beta=0.0, rbias=True),
    _k(alpha=1.0, beta=0.0, relu=True),
    _k(alpha=1.0, beta=0.25),
    _k(alpha=1.0, beta=1.0),
    _k(alpha=0.5, beta=0.0),
    _k(alpha=-2.0, beta=0.0),
    _k(alpha=-2.0, beta=0.25, bias=True, rbias=True, relu=True),
    _k(alpha=0.5, beta=1.0, bias=True, rbias=True, relu=True),
    _k(alpha=1.0, beta=0.0, bias=True, rbias=True, relu=True),
    _k(alpha=0.0, beta=0.5, bias=True),
)
EPILOGUE_SHAPE = (77, 45, 133)

# split-K: one output tile, K = 256 s (and 256 s - 5: a ragged last slice); the planner is expected to cut it into s
# slices of 256 (the tests assert the count the library reports)
SPLIT_COUNTS = tuple(range(2, 18)) + (24,)
SPLIT_RAGGED = (2, 7, 8, 9)
SPLIT_SWEEP = tuple((60, 45, 256 * s, s) for s in SPLIT_COUNTS) + tuple((60, 45, 256 * s - 5, s) for s in SPLIT_RAGGED)
SPLIT_EPILOGUE_COUNTS = (3, 8, 13)
# (M, N, aligned): float4 slabs + float4 C / float4 slabs + scalar C / all scalar
SPLIT_EPILOGUE_SHAPES = ((60, 44, True), (60, 45, False), (33, 45, False))
SHORT_WS = (60, 45, 1024)
MULTI_TILE_SPLIT = (192, 192, 1024)

MIXED_BATCH = (
    _k(M=33, N=45, K=1792, alpha=0.5, beta=0.25, bias=True),               # split, scalar reduce (M N odd)
    _k(M=60, N=44, K=1792, alpha=-2.0, beta=1.0, rbias=True, relu=True, aligned=True),  # split, slabs at an odd offset
    _k(M=64, N=64, K=96, alpha=1.0, beta=0.0, bias=True, rbias=True, relu=True),        # unsplit: the tile kernel
    _k(M=10, N=7, K=0, alpha=0.25, beta=0.5, bias=True),                   # K = 0
    _k(M=0, N=5, K=64, alpha=1.0, beta=1.0),                               # skipped
)
SIXTEEN = tuple(_k(M=3 + 5 * i, N=2 + 3 * ((7 * i) % 16), K=1 + 9 * ((5 * i) % 16), bias=bool(i & 1), rbias=bool(i & 2),
                   relu=bool(i & 4) and bool(i & 3)) for i in range(16))

PRECISION = (
    ((77, 45, 133), FORMS),
    ((256, 384, 512), ((0, 1), (1, 0))),
    ((64, 64, 8192), ((0, 1), (1, 0))),   # split-K
    ((60, 45, 4352), ((0, 1), (1, 0))),
)
PRECISION_OPTIONS = _k(alpha=0.5, beta=0.25, bias=True, data="random")


# ------------------------------------------------------------------------------------- the bf16 tile family's tables
# gemm_bf16_kernel<TA, TB, BM, BN> (csrc/gemm_f32.hip) runs every exact table above; its own additions follow.
BF16_KTILE = 64
BF16_SINGLE_SHAPES = SINGLE_SHAPES + (
    (64, 64, 64), (64, 64, 128),   # whole 64-deep K-tiles: the unguarded loader only
    (64, 64, 63), (64, 64, 65),    # one short of a K-tile, and one past it: the guarded loader
)
# Mread / Nread exist for the unguarded loader, which gemm_bf16_kernel takes only when the tile lies within the
# declared padding AND its K range is whole K-tiles of 64 (PADDED's K = 96 is whole tiles for the fp32 kernel's 32
# only: under bf16 it runs the guarded loader, which ignores the declaration).  These reach it: one K-tile and two,
# each declaration alone and both together, and a second row tile that alone straddles M.
BF16_PADDED = (_k(M=64, N=40, K=64, Nread=64), _k(M=40, N=64, K=128, Mread=64),
               _k(M=40, N=40, K=64, Mread=64, Nread=64), _k(M=104, N=64, K=128, Mread=128))
# (M, N, K, bm, bn): plan_gemm takes the wider tile only when at least 256 of them exist
BF16_WIDE_TILES = (
    (2048, 2048, 64, 128, 128),    # 256 whole tiles
    (2050, 2040, 100, 128, 128),   # 17 x 16 tiles, ragged on every edge
    (64, 32768, 64, 64, 128),      # every problem has M <= 64: 64 x 128, 256 whole tiles
    (40, 32700, 100, 64, 128),     # ragged on every edge
)


def bf16_tile_plan(shapes, ws_floats):
    """plan_gemm's bf16 branch (csrc/gemm_f32.hip) restated: (M, N, K) of the problems with M, N > 0 and the workspace
    floats -> (bm, bn, kslice, nblocks, [splits per problem]).  The halving rule: while the output has fewer than 512
    tiles and the launch fewer than 1024 blocks, halve the K slice (rounded up to whole K-tiles of 64), down to 256
    (fewer than 256 tiles) or 512, and only while the slabs fit the workspace."""
    kq = BF16_KTILE
    kfull = (max(K for _, _, K in shapes) + kq - 1) // kq * kq

    def count(bm, bn, ks):
        blocks, slab = 0, 0
        for M, N, K in shapes:
            sp = -(-K // ks) if K > 0 and ks > 0 else 1
            blocks += -(-M // bm) * -(-N // bn) * sp
            slab += sp * M * N if sp > 1 else 0
        return blocks, slab <= ws_floats

    bm, bn, ks = 64, 64, kfull
    blocks, _ = count(bm, bn, ks)
    wide = (64 if max(M for M, _, _ in shapes) <= 64 else 128, 128)
    if count(*wide, ks)[0] >= 256:
        bm, bn = wide
        blocks = count(bm, bn, ks)[0]
    tiles = blocks
    kmin = 256 if tiles < 256 else 512
    while tiles < 512 and blocks < 1024 and ks // 2 >= kmin:
        nx = (ks // 2 + kq - 1) // kq * kq
        nb, fits = count(bm, bn, nx)
        if not fits:
            break
        ks, blocks = nx, nb
    return bm, bn, ks, blocks, [(-(-K // ks) if K > 0 and ks > 0 else 1) for _, _, K in shapes]


# bf16 split-K follows the halving rule, not the fp32 search, so its table is its own: (M, N, K, splits, kslice) as
# bf16_tile_plan gives them with the full workspace (checked on the CPU), which the GPU tests assert from the
# library's record.  2, 4, 8 and 16 slices; K = 768, 1536 and 6144 end at slices of 384 (not a power of two);
# K = 1019 and 4091 leave a ragged last slice (251 of 256); K = 3328 goes 1664, 832, 448 (416 rounded up to whole
# K-tiles) and leaves a last slice of 192.  (64, 64, 1024) is a whole tile: its slices 1..3 start at kbeg != 0 on the
# unguarded loader.
BF16_SPLIT_SWEEP = (
    (60, 45, 512, 2, 256), (60, 45, 768, 2, 384), (60, 45, 1024, 4, 256), (60, 45, 1019, 4, 256),
    (60, 45, 1536, 4, 384), (60, 45, 2048, 8, 256), (60, 45, 3328, 8, 448), (60, 45, 4096, 16, 256),
    (60, 45, 4091, 16, 256), (60, 45, 6144, 16, 384), (64, 64, 1024, 4, 256),
)
BF16_WS_FLOATS = 8 << 20  # kGemmWsFloats: what the GPU tests pass

# the precision leg on normal data, a few shapes only: 64 x 64 tiles with every edge ragged, the 128 x 128 tile, and
# a split (8192 -> 32 slices of 256)
BF16_PRECISION = (
    ((77, 45, 133), FORMS),
    ((2050, 2040, 100), ((0, 1), (1, 0))),
    ((64, 64, 8192), ((0, 1), (1, 0))),
)
# the rounding leg: one whole K-tile on the unguarded loader, a K = 40 tail on the guarded one
BF16_ROUNDING = (_k(M=64, N=64, K=64), _k(M=77, N=45, K=40, bias=True, beta=0.25), _k(M=64, N=128, K=64, relu=True, rbias=True))


def bf16_exact_case_args():
    """(tA, tB, kwargs) of every exact-data case the bf16 tile family runs: the fp32 tables and its own."""
    out = list(exact_case_args())
    for tA, tB in FORMS:
        for M, N, K in BF16_SINGLE_SHAPES[len(SINGLE_SHAPES):]:
            out.append((tA, tB, _k(M=M, N=N, K=K)))
        for M, N, K, _, _ in BF16_WIDE_TILES:
            out.append((tA, tB, _k(M=M, N=N, K=K)))
        for p in BF16_PADDED:
            out.append((tA, tB, p))
            out.append((tA, tB, dict(p, Mread=0, Nread=0)))
    for tA, tB in SPLIT_FORMS:
        for M, N, K, _, _ in BF16_SPLIT_SWEEP:
            out.append((tA, tB, _k(M=M, N=N, K=K)))
    return out


def bf16_precision_case_args():
    return [(tA, tB, _k(M=M, N=N, K=K, **PRECISION_OPTIONS)) for (M, N, K), forms in BF16_PRECISION for tA, tB in forms]


def exact_case_args():
    """(tA, tB, kwargs) of every exact-data case of the tables above."""
    out = []
    for tA, tB in FORMS:
        for M, N, K in SINGLE_SHAPES + EMPTY_SHAPES:
            out.append((tA, tB, _k(M=M, N=N, K=K)))
        for o in K0_OPTIONS:
            out.append((tA, tB, _k(M=40, N=33, K=0, **o)))
        for p in PADDED:
            out.append((tA, tB, p))
            out.append((tA, tB, dict(p, Mread=0, Nread=0)))
        for o in EPILOGUES:
            M, N, K = EPILOGUE_SHAPE
            out.append((tA, tB, _k(M=M, N=N, K=K, **o)))
    for tA, tB in SPLIT_FORMS:
        for M, N, K, _ in SPLIT_SWEEP:
            out.append((tA, tB, _k(M=M, N=N, K=K)))
        for s in SPLIT_EPILOGUE_COUNTS:
            for M, N, al in SPLIT_EPILOGUE_SHAPES:
                for o in EPILOGUES:
                    out.append((tA, tB, _k(M=M, N=N, K=256 * s, aligned=al, **o)))
        for M, N, K in (SHORT_WS, MULTI_TILE_SPLIT):
            out.append((tA, tB, _k(M=M, N=N, K=K)))
        for p in MIXED_BATCH + SIXTEEN:
            out.append((tA, tB, p))
    return out


def precision_case_args():
    return [(tA, tB, _k(M=M, N=N, K=K, **PRECISION_OPTIONS)) for (M, N, K), forms in PRECISION for tA, tB in forms]
