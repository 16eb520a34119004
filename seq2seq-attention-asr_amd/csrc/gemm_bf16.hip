// Large bf16 GEMMs on gfx950 MFMA, in house (the module-level products of the bf16 modes: the VGG front-end's
// 1x1 TemporalConvolution layers, librispeech/model_vgg.lua:45-52, M = B L' ~ 8128 rows x 2048 x 896..2048, their
// input and weight gradients, and the attention decoder's Vh / dh / weight-gradient products under that model,
// Attention.lua:43-47).  Replaces the vendor library for these shapes.
//
// Row-major C (M x N) = alpha op(A) op(B) (+ bias[n]) (+ beta C) (ReLU) -- the GemmProblem contract.
//  1. Staging: each fp32 operand is rounded to bf16 (RNE) into a K-contiguous copy [R][Kp] (K zero-padded to the
//     K-tile) in the calling context's staging buffer (one pass; a transposed operand goes through a 64 x 64 LDS
//     tile), so the main loop reads one layout with no guards: A' [M][Kp], B' [N][Kp], C = A' B'^T; tile rows past
//     M / N read the last row and are never stored.
//  2. gemm_bf16_nt: a BM x BN x 64 tile per workgroup, waves WM x WN, each a (BM/WM) x (BN/WN) block of
//     v_mfma_f32_16x16x32_bf16 accumulators.  K-tiles are staged global -> LDS by global_load_lds_dwordx4
//     (LDS-DMA, no register pass), two LDS stages: the next tile's DMA is issued before the current tile's
//     fragment reads and MFMAs, one vmcnt(0) + barrier per K-tile (cdna_hip_programming.md §5, "Minimum
//     2-phase").  The LDS image is lane-linear per 1-KB wave instruction (8 rows x 128 B), so the bank swizzle is
//     applied on the SOURCE address: row r's 16-B chunk p holds k-chunk p ^ ((r >> 1) & 7), and the fragment
//     reads (16 rows x one k-chunk per 16-lane group) hit 16 distinct 16-B slots of the 256-B bank row.
//     All LDS lives in one dynamic array (a second __shared__ object made hipcc drain vmcnt early, guide §5 4a).
//  3. Output tiles are dealt XCD-contiguously (bijective remap), the N tiles of one M panel next to each other
//     (the A' panel is shared through that XCD's L2).  Too few tiles for the chip: split-K into S slices, each
//     writing an fp32 slab, summed in slice order by bf16_splitk_reduce (deterministic), which applies the
//     epilogue.
// The result equals a float64 product of the bf16-rounded operands to fp32-accumulation accuracy
// (tests/test_gpu_bf16.py), like the other bf16 kernels of the library.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "s2s_common.h"

namespace s2s {

// ------------------------------------------------------------------ the context-owned staging buffer
thread_local GemmStage* t_stage = nullptr;  // the calling context's staging buffer (set_gemm_stage, per C-ABI call)
void set_gemm_stage(GemmStage* s) { t_stage = s; }
void gemm_stage_free(GemmStage* s) {
  if (!s) return;
  for (int i = 0; i < GemmStage::kStreams; ++i) {
    if (s->p[i]) (void)hipFree(s->p[i]);
    s->p[i] = s->s[i] = nullptr;
    s->n[i] = 0;
  }
  for (void* q : s->old) (void)hipFree(q);
  s->old.clear();
}

std::atomic<int> g_gemm_big{1};     // s2s_debug_gemm_big(0): these problems stay on gemm_f32's 64 x 64 bf16 tiles
std::atomic<long> g_big_calls{0};   // big-GEMM calls launched (s2s_debug_gemm_big_calls)

// the calling context's staging buffer for stream `st` with at least `bytes`, or nullptr (no context, more streams
// than slots, or too small while capturing)
void* stage_acquire(hipStream_t st, size_t bytes) {
  GemmStage* s = t_stage;
  if (!s) return nullptr;
  int k = -1;
  for (int i = 0; i < GemmStage::kStreams && k < 0; ++i)
    if (s->p[i] && s->s[i] == static_cast<void*>(st)) k = i;
  if (k >= 0 && s->n[k] >= bytes) return s->p[k];
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
  if (k < 0)
    for (int i = 0; i < GemmStage::kStreams && k < 0; ++i)
      if (!s->p[i]) k = i;
  if (k < 0) {  // every slot holds another stream's buffer: the caller falls back to the 64 x 64 tile GEMM
    static std::atomic<int> warned{0};
    if (!warned.exchange(1))
      std::fprintf(stderr, "s2s: bf16 GEMM staging slots exhausted (%d streams); big GEMMs on further streams use "
                           "the 64x64 tiles\n", GemmStage::kStreams);
    return nullptr;
  }
  void* p = nullptr;
  const size_t want = std::max(bytes, s->n[k] * 2);
  if (hipMalloc(&p, want) != hipSuccess) return nullptr;
  if (s->p[k]) s->old.push_back(s->p[k]);
  s->p[k] = p;
  s->s[k] = static_cast<void*>(st);
  s->n[k] = want;
  return p;
}

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_void_t;
typedef __attribute__((address_space(1))) const void* glb_void_t;

constexpr int kBK = 64;  // K-tile (bf16): 128-byte LDS rows

// ---- staging: logical operand (R x K), element (r, k) at src[r * ld + k] -> dst [R][Kp] bf16, K zero padded (rows
// are not padded: the GEMM's DMA reads row R - 1 for tile rows past R, and never stores them).
// One thread per 8 consecutive k of a row: two float4 loads, one 16-byte store.
__global__ __launch_bounds__(256) void stage_kc_bf16(const float* __restrict__ src, long ld, int R, int K, int Kp,
                                                     long n8, int vec, __bf16* __restrict__ dst) {
  const int kq = Kp / 8;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const long r = i / kq;
    const int k = (int)(i - r * kq) * 8;
    floatx4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (r < R) {
      const float* row = src + r * ld;
      if (vec && k + 8 <= K) {
        a = *reinterpret_cast<const floatx4*>(row + k);
        b = *reinterpret_cast<const floatx4*>(row + k + 4);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = k + j < K ? row[k + j] : 0.f;
          b[j] = k + 4 + j < K ? row[k + 4 + j] : 0.f;
        }
      }
    }
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (__bf16)a[j];
      v[4 + j] = (__bf16)b[j];
    }
    *reinterpret_cast<bf16x8*>(dst + r * Kp + k) = v;
  }
}

// transposed operand: element (r, k) at src[k * ld + r] (row-contiguous along r) -> dst [R][Kp]; one 64 (r) x 64 (k)
// tile per workgroup through LDS (coalesced reads along r, 16-byte writes along k)
__global__ __launch_bounds__(256) void stage_rc_bf16(const float* __restrict__ src, long ld, int R, int K, int Kp,
                                                     __bf16* __restrict__ dst) {
  __shared__ float t[64][65];
  const int r0 = blockIdx.x * 64, k0 = blockIdx.y * 64, tid = threadIdx.x;
  const int rr = r0 + (tid & 63);
  for (int kk = tid >> 6; kk < 64; kk += 4) {
    const int k = k0 + kk;
    t[kk][tid & 63] = (k < K && rr < R) ? src[(long)k * ld + rr] : 0.f;
  }
  __syncthreads();
  for (int c = tid; c < 512; c += 256) {
    const int r = c >> 3, kc = (c & 7) * 8;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)t[kc + j][r];
    if (r0 + r < R) *reinterpret_cast<bf16x8*>(dst + (long)(r0 + r) * Kp + k0 + kc) = v;
  }
}

// ---- the GEMM
struct BigGemm {
  const __bf16* A;  // [M][Kp]
  const __bf16* B;  // [N][Kp]
  float* C;
  const float* bias;
  float* part;      // split-K slabs [S][M][N] or nullptr
  long ldc;
  int M, N, Kp, kslice;  // kslice: K-tiles per split (all of them when S = 1)
  int tiles_m, tiles_n, S, nblocks;
  float alpha, beta;
  int relu;
};

// bijective XCD-contiguous remap of a 1-D grid (hardware deals blockIdx round-robin over the 8 XCDs)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8, x = bid % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
}

// LDS byte offset of (row, k-chunk c) in a [rows][128 B] image whose chunks are swizzled by (row >> 1) & 7
__device__ __forceinline__ int swz(int row, int c) { return row * 128 + ((c ^ ((row >> 1) & 7)) << 4); }

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void gemm_bf16_nt(BigGemm g) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  constexpr int GA = BM / 8 / NW, GB = BN / 8 / NW;  // 1-KB DMA instructions per wave per K-tile
  constexpr int STAGE = (BM + BN) * 128;             // bytes of one LDS stage
  static_assert(GA >= 1 && GB >= 1 && BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile / wave split");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  if (lin >= g.nblocks) return;
  const int tn = lin % g.tiles_n, rest = lin / g.tiles_n, tm = rest % g.tiles_m, s = rest / g.tiles_m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kt0 = s * g.kslice, nk = min(g.kslice, g.Kp / kBK - kt0);

  // DMA sources: wave instruction j covers rows 8 (wave + NW j) .. + 7 of the tile; lane l -> row + (l >> 3),
  // LDS chunk l & 7 <- k-chunk (l & 7) ^ swizzle(row)
  const __bf16* asrc[GA];
  const __bf16* bsrc[GB];
#pragma unroll
  for (int j = 0; j < GA; ++j) {
    const int row = 8 * (wave + NW * j) + (lane >> 3);  // rows past M read row M - 1 (never stored)
    asrc[j] = g.A + (long)min(m0 + row, g.M - 1) * g.Kp + (long)kt0 * kBK + 8 * ((lane & 7) ^ ((row >> 1) & 7));
  }
#pragma unroll
  for (int j = 0; j < GB; ++j) {
    const int row = 8 * (wave + NW * j) + (lane >> 3);
    bsrc[j] = g.B + (long)min(n0 + row, g.N - 1) * g.Kp + (long)kt0 * kBK + 8 * ((lane & 7) ^ ((row >> 1) & 7));
  }
  auto stage = [&](int kt, int buf) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int j = 0; j < GA; ++j)
      __builtin_amdgcn_global_load_lds((glb_void_t)(asrc[j] + (long)kt * kBK),
                                       (lds_void_t)(base + 1024 * (wave + NW * j)), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < GB; ++j)
      __builtin_amdgcn_global_load_lds((glb_void_t)(bsrc[j] + (long)kt * kBK),
                                       (lds_void_t)(base + BM * 128 + 1024 * (wave + NW * j)), 16, 0, 0);
  };

  floatx4 acc[FM][FN];
#pragma unroll
  for (int f = 0; f < FM; ++f)
#pragma unroll
    for (int q = 0; q < FN; ++q) acc[f][q] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lq = lane >> 4;
  if (nk > 0) {
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nk) stage(kt + 1, buf ^ 1);  // the next tile's DMA runs under this tile's MFMAs
      const char* As = smem + buf * STAGE;
      const char* Bs = As + BM * 128;
#pragma unroll
      for (int ks = 0; ks < kBK / 32; ++ks) {
        bf16x8 a[FM], b[FN];
#pragma unroll
        for (int f = 0; f < FM; ++f) {
          const int row = wm * TM + 16 * f + lr;
          a[f] = *reinterpret_cast<const bf16x8*>(As + swz(row, 4 * ks + lq));
        }
#pragma unroll
        for (int q = 0; q < FN; ++q) {
          const int row = wn * TN + 16 * q + lr;
          b[q] = *reinterpret_cast<const bf16x8*>(Bs + swz(row, 4 * ks + lq));
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int f = 0; f < FM; ++f)
#pragma unroll
          for (int q = 0; q < FN; ++q) acc[f][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[f], b[q], acc[f][q], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next stage has landed ...
      __syncthreads();                                  // ... and every wave is done with this one
    }
  }

  // epilogue (16 x 16 accumulator map: column lane & 15, rows 4 (lane >> 4) + r)
#pragma unroll
  for (int f = 0; f < FM; ++f)
#pragma unroll
    for (int q = 0; q < FN; ++q) {
      const int col = n0 + wn * TN + 16 * q + lr;
      if (col >= g.N) continue;
      const bool has_bias = !g.part && g.bias;  // (no bias: nothing is added, so -0 stays -0 as in the reduce)
      const float bv = has_bias ? g.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * TM + 16 * f + 4 * lq + r;
        if (row >= g.M) continue;
        if (g.part) {
          g.part[((long)s * g.M + row) * g.N + col] = acc[f][q][r];
        } else {
          float v = g.alpha * acc[f][q][r];
          if (has_bias) v += bv;
          float* c = g.C + (long)row * g.ldc + col;
          if (g.beta != 0.f) v += g.beta * *c;
          if (g.relu) v = fmaxf(v, 0.f);
          *c = v;
        }
      }
    }
}

// C = alpha * (sum of the S slabs in slice order) (+ bias) (+ beta C) (ReLU)
__global__ __launch_bounds__(256) void bf16_splitk_reduce(BigGemm g) {
  const long mn = (long)g.M * g.N;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < mn; e += (long)gridDim.x * 256) {
    float v[16];
    float sum = 0.f;
    int s = 0;
    for (; s + 16 <= g.S; s += 16) {  // sixteen slabs' loads in flight, summed in order
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = g.part[(s + j) * mn + e];
#pragma unroll
      for (int j = 0; j < 16; ++j) sum += v[j];
    }
    for (; s < g.S; ++s) sum += g.part[s * mn + e];
    const long row = e / g.N;
    const int col = (int)(e - row * g.N);
    float o = g.alpha * sum;
    if (g.bias) o += g.bias[col];
    float* c = g.C + row * g.ldc + col;
    if (g.beta != 0.f) o += g.beta * *c;
    if (g.relu) o = fmaxf(o, 0.f);
    *c = o;
  }
}


template <int BM, int BN, int WM, int WN>
int launch_nt(hipStream_t st, const BigGemm& g) {
  const size_t lds = 2 * (size_t)(BM + BN) * 128;
  static std::atomic<int> attr_set{0};
  if (!attr_set.load(std::memory_order_relaxed)) {
    S2S_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_nt<BM, BN, WM, WN>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set.store(1, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL((gemm_bf16_nt<BM, BN, WM, WN>), dim3((unsigned)g.nblocks), dim3(WM * WN * 64), lds, st, g);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

bool gemm_big_enabled() { return g_gemm_big != 0; }

static thread_local GemmBigLastPlan t_big_last;
const GemmBigLastPlan& gemm_big_last_plan() { return t_big_last; }
static thread_local int t_force_bm = 0, t_force_bn = 0, t_force_s = 0;  // gemm_big_force
bool gemm_big_force(int bm, int bn, int splits) {
  const bool tile = (bm == 0 && bn == 0) || (bm == 256 && bn == 256) || (bm == 256 && bn == 128) || (bm == 128 && bn == 128);
  if (!tile || splits < 0 || splits > 256) return false;
  t_force_bm = bm;
  t_force_bn = bn;
  t_force_s = splits;
  return true;
}

int gemm_big_bf16(hipStream_t st, const GemmProblem& q, bool transA, bool transB, bool* done) {
  *done = false;
  GemmBigLastPlan& rec = t_big_last;
  rec = GemmBigLastPlan{};
  rec.declined = 1;
  if (!g_gemm_big || !t_stage || q.M <= 0 || q.N <= 0 || q.K <= 0 || q.rbias || q.Mread || q.Nread) return 0;
  const int M = q.M, N = q.N, K = q.K, Kp = (K + kBK - 1) / kBK * kBK, nkt = Kp / kBK;
  // Tile and split-K from a time model: per-CU rates of the three tiles (measured on MI355X, tools/gemm_big_bench.py:
  // 256 x 256 ~3.9, 256 x 128 ~2.9, 128 x 128 ~1.6 TFLOP/s per CU at one workgroup per CU -- the 128 x 128 tile is
  // bound by its 64 B/clk of staged operands), whole waves of 256 workgroups, and a split's slab round trip (write +
  // read of S M N floats at ~5 TB/s) plus the reduce launch.
  struct Cand { int bm, bn; double rate; };
  const Cand cands[3] = {{256, 256, 3.9e12}, {256, 128, 2.9e12}, {128, 128, 1.6e12}};
  double best = 1e30;
  int BM = 128, BN = 128, S = 1;
  for (const Cand& c : cands) {
    const long tl = (long)((M + c.bm - 1) / c.bm) * ((N + c.bn - 1) / c.bn);
    for (int s = 1; s <= 256; s *= 2) {  // (the first VGG layer's 64 x 27 weight gradient: K = 621k pixels)
      if (s > 1 && nkt / s < 4) break;  // >= 4 K-tiles per slice
      const int ks = (nkt + s - 1) / s;
      const long blocks = tl * ((nkt + ks - 1) / ks);
      const double waves = std::ceil(blocks / 256.0);
      double t = waves * 2.0 * c.bm * c.bn * (double)ks * kBK / c.rate;
      if (s > 1) t += 2.0 * s * (double)M * N * 4.0 / 5e12 + 3e-6;
      if (t < best * 0.98) { best = t; BM = c.bm; BN = c.bn; S = s; }
    }
  }
  if (t_force_bm) { BM = t_force_bm; BN = t_force_bn; }  // test override: the same kernels, chosen by hand
  if (t_force_s) S = t_force_s;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN, tiles = tiles_m * tiles_n;
  const int kslice = (nkt + S - 1) / S;
  S = (nkt + kslice - 1) / kslice;
  // (the override never runs another count than the one asked for: nothing is launched)
  S2S_REQUIRE(!t_force_s || S == t_force_s, "gemm_big_bf16: the forced split count does not divide this problem's " +
                                                std::to_string(nkt) + " K-tiles into that many slices");
  const size_t abytes = (size_t)M * Kp * 2, bbytes = (size_t)N * Kp * 2;
  const size_t slab = S > 1 ? sizeof(float) * (size_t)S * M * N : 0;
  const size_t off_b = (abytes + 255) / 256 * 256, off_p = off_b + (bbytes + 255) / 256 * 256;
  char* stg = static_cast<char*>(stage_acquire(st, off_p + slab));
  if (!stg) return 0;
  __bf16* Ah = reinterpret_cast<__bf16*>(stg);
  __bf16* Bh = reinterpret_cast<__bf16*>(stg + off_b);
  // operands -> [M][Kp] / [N][Kp] (A: element (m, k) at A[m lda + k], or A[k lda + m] when transA; B: (n, k) at
  // B[n ldb + k] when transB (the NT form), else B[k ldb + n])
  auto stage_op = [&](const float* src, long ld, int R, bool rowc, __bf16* dst, int* how) -> int {
    if (rowc) {
      hipLaunchKernelGGL(stage_rc_bf16, dim3((R + 63) / 64, Kp / 64), dim3(256), 0, st, src, ld, R, K, Kp, dst);
      *how = kStageRc;
    } else {
      const long n8 = (long)R * Kp / 8;
      const int vec = (ld % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) ? 1 : 0;
      const unsigned blocks = (unsigned)std::min<long>(4096, (n8 + 255) / 256);
      hipLaunchKernelGGL(stage_kc_bf16, dim3(blocks), dim3(256), 0, st, src, ld, R, K, Kp, n8, vec, dst);
      *how = vec ? kStageKcVec : kStageKcScalar;
    }
    S2S_CHECK_HIP(hipGetLastError());
    return 0;
  };
  S2S_TRY(stage_op(q.A, q.lda, M, transA, Ah, &rec.stage_a));
  S2S_TRY(stage_op(q.B, q.ldb, N, !transB, Bh, &rec.stage_b));
  BigGemm g{};
  g.A = Ah;
  g.B = Bh;
  g.C = q.C;
  g.bias = q.bias;
  g.part = S > 1 ? reinterpret_cast<float*>(stg + off_p) : nullptr;
  g.ldc = q.ldc;
  g.M = M;
  g.N = N;
  g.Kp = Kp;
  g.kslice = kslice;
  g.tiles_m = tiles_m;
  g.tiles_n = tiles_n;
  g.S = S;
  g.nblocks = tiles * S;
  g.alpha = q.alpha;
  g.beta = q.beta;
  g.relu = q.relu;
  {
    ProfScope ps(st, "gemm_big_bf16", 2.0 * M * (double)N * K,
                 4.0 * ((double)M * K + (double)K * N + (double)M * N * (q.beta != 0.f ? 2 : 1)));
    if (BM == 256 && BN == 256) S2S_TRY((launch_nt<256, 256, 2, 4>(st, g)));
    else if (BM == 256) S2S_TRY((launch_nt<256, 128, 4, 2>(st, g)));
    else S2S_TRY((launch_nt<128, 128, 2, 2>(st, g)));
  }
  if (S > 1) {
    const long mn = (long)M * N;
    hipLaunchKernelGGL(bf16_splitk_reduce, dim3((unsigned)std::min<long>(2048, (mn + 255) / 256)), dim3(256), 0, st, g);
    S2S_CHECK_HIP(hipGetLastError());
  }
  rec.launched = 1;
  rec.declined = 0;
  rec.bm = BM;
  rec.bn = BN;
  rec.S = S;
  rec.kslice = kslice;
  rec.nblocks = g.nblocks;
  rec.forced = (t_force_bm || t_force_s) ? 1 : 0;
  *done = true;
  ++g_big_calls;
  return 0;
}

}  // namespace s2s

extern "C" void s2s_debug_gemm_big(int on) { s2s::g_gemm_big = on; }
// test override of the big GEMM's tile and split count on the calling thread (gemm_big_force; 0, 0, 0 = the time
// model); 0 when accepted, 1 when refused (nothing changes)
extern "C" int s2s_debug_gemm_big_force(int bm, int bn, int splits) { return s2s::gemm_big_force(bm, bn, splits) ? 0 : 1; }
// the record of the calling thread's last gemm_big_bf16 call (GemmBigLastPlan, field by field)
struct s2s_debug_gemm_big_plan {
  int launched, declined, bm, bn, S, kslice, nblocks, stage_a, stage_b, forced;
};
extern "C" void s2s_debug_gemm_big_last(s2s_debug_gemm_big_plan* out) {
  const s2s::GemmBigLastPlan& p = s2s::gemm_big_last_plan();
  if (out) *out = s2s_debug_gemm_big_plan{p.launched, p.declined, p.bm, p.bn, p.S, p.kslice, p.nblocks, p.stage_a,
                                           p.stage_b, p.forced};
}
extern "C" long s2s_debug_gemm_big_calls() { return s2s::g_big_calls; }
