// XCD-local attention-decoder recurrences (included by attn.hip inside its anonymous namespace,
// after attn_persist.inc).
//
// Same model as the per-step kernels (Attention.lua:51-184, RNNAttention.lua:144-253), regrouped
// so that each decoder step has 5 hand-off seams instead of 7 and every seam stays inside one
// XCD's L2:
//
//  * Teacher forcing makes every y-dependent term known before the loop, and d enters the decoder
//    GRU only linearly, so the c -> c_in -> d -> gate chain folds into ONE product with weights
//    fixed for the call (dec_xcd_prologue):
//        Wx' = [Wz_d; Wr_d; Wh_d] . Wd_c . Wc   (3S x A)      [W*_d = W*[:, S:], Wd_c = Wd[:, :S]]
//        KX_t = [Wz_d; Wr_d; Wh_d] . (Wd_c bc + Wd_y y_in_t + bd)   (3S per (b, t))
//    so the gates' d-part is Wx' c_t + KX_t (Attention.lua:149-152, GRU.lua:22-26).  Backward
//    mirrors it: dc_t = Wx'^T [da_z; da_r; da_h] + dc_mlp.  dd, [dc_in | dy_in], c_in and d are
//    recomputed for the weight gradients by GEMMs over all B*T rows after the loop.
//  * A chain = U utterances on kXWG = 32 workgroups (one per CU) of ONE XCD (chain_slot /
//    chain_is_local, handoff.h): granules stay in that XCD's L2 (0.22 us per hop).  Each
//    workgroup owns one 32-frame attention chunk of one utterance for the whole launch, its h and
//    Vh rows resident in LDS (U * ceil(L/32) <= 32).
//  * Backward keeps no per-frame accumulators in the loop: it saves de_{t,l} and dc_t; dh and
//    dVh / dwe are contractions over t done after the loop (dec_xcd_dvh + one batched GEMM).
//
// Forward step t (seams marked |):   F1 ws, us = Ws s + bs, [Wz_s; Wr_s] s  |  F2 attention chunk
//   |  F3 combine -> c  |  F4 gx = Wx' c + KX -> z, r, q = r s  |  F5 hh, s_t  |
// Backward step t:  G gate grads (da_z, da_h)  |  B2 dq = Wh_s^T da_h -> da_r  |  B3 dc =
//   Wx'^T da + dc_mlp, us' = [Wz_s; Wr_s]^T [da_z; da_r]  |  B4 attention chunk -> partial dws
//   |  B45 dws = sum of chunks  |  B5 ds_{t-1} = ds(1-z) + dq r + us' + Ws^T dws + ds_mlp -> G(t-1)


// tanh(x) = 1 - 2 / (exp(2x) + 1) on v_exp_f32 / v_rcp_f32: ~1e-7 absolute error, saturates to +-1,
// a few instructions instead of libm tanhf's ~30 (the attention phases evaluate 2 * 16K per step)
__device__ __forceinline__ float tanh_fast(float v) {
  return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * v) + 1.f);
}
// The attention sums over (frame, score column) in factored form: with zk = K z (K = 2 log2 e, folded into the
// ws operand so that zk = fma(Vh, K, K ws) is one instruction) and r = 1 / (2^zk + 1), tanh z = 1 - 2 r and
// 1 - tanh^2 z = 4 r (1 - r).  A score sum_j we_j tanh z_j is then sum_j we_j - 2 sum_j we_j r_j (the first a
// per-launch constant), and each term costs fma, v_exp, add, v_rcp, fma instead of tanh_fast's seven
// instructions plus the product.
constexpr float kTanhK = 2.8853900817779268f;
__device__ __forceinline__ float tanh_r(float zk) { return __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(zk) + 1.f); }

// Product form of the attention terms: with E_lj = 2^(K Vh_lj) (staged in LDS in place of the Vh rows, once per
// launch) and W_j = 2^(K ws_j) (once per column and step), r = 1 / (E W + 1): one v_rcp and one fma per term instead
// of an fma, v_exp, add and v_rcp.  Exact in the limits: a product that overflows gives r = 0 (tanh = 1) and one that
// underflows (or is flushed) r = 1 (tanh = -1), which is what fp32 tanh returns there (|K z| > 126 -- with |K Vh| <=
// kPfMax the product leaves the normal range only there) -- as long as E itself is finite and normal.  So a chunk
// whose rows hold any |K Vh| > kPfMax (or a NaN) keeps the per-term form for the launch (a workgroup-uniform flag set
// while staging; s2s_debug_dec_pf(0) forces it everywhere).  The streamed levels (RES = 0) form E from the loaded Vh
// with the same instruction, so every level stays bitwise equal.
__device__ int g_dec_pf = 1;
constexpr float kPfMax = 100.f;
__device__ __forceinline__ float pf_e(float v) { return __builtin_amdgcn_exp2f(kTanhK * v); }
__device__ __forceinline__ float4 pf_e4(float4 v) { return make_float4(pf_e(v.x), pf_e(v.y), pf_e(v.z), pf_e(v.w)); }
__device__ __forceinline__ bool pf_wide(float4 v) {
  return !(fabsf(kTanhK * v.x) <= kPfMax) || !(fabsf(kTanhK * v.y) <= kPfMax) || !(fabsf(kTanhK * v.z) <= kPfMax) ||
         !(fabsf(kTanhK * v.w) <= kPfMax);
}
// Check the chunk's n4v float4 of Vh rows (vs) and stage them into vdst (RES > 0) as E (product form) or as Vh; all
// threads of an attention workgroup call it (it ends on a barrier); *wide_lds starts at 0 (1: per-term form forced).
// Returns the workgroup's form: true = product.
// Both passes keep eight float4 loads per thread in flight (a one-at-a-time loop -- and the short-circuit check, whose
// every load waited on the previous one's test -- made the staging half of the launch prologue: 10.5 of 18 us at
// config 2, 20 of 34 at config 4).
template <int RES>
__device__ __forceinline__ bool stage_vh(float4* vdst, const float4* vs, int n4v, int* wide_lds) {
  bool wide = false;
  int i = threadIdx.x;
  for (; i + 7 * 256 < n4v; i += 8 * 256) {
    float4 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = vs[i + q * 256];
#pragma unroll
    for (int q = 0; q < 8; ++q) wide |= pf_wide(v[q]);
  }
  for (; i < n4v; i += 256) wide |= pf_wide(vs[i]);
  if (wide) *wide_lds = 1;
  __syncthreads();
  const bool pf = *wide_lds == 0;
  if (RES > 0) {
    i = threadIdx.x;
    for (; i + 7 * 256 < n4v; i += 8 * 256) {
      float4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = vs[i + q * 256];
#pragma unroll
      for (int q = 0; q < 8; ++q) vdst[i + q * 256] = pf ? pf_e4(v[q]) : v[q];
    }
    for (; i < n4v; i += 256) vdst[i] = pf ? pf_e4(vs[i]) : vs[i];
  }
  return pf;
}
// n elements loaded by ld(i) and stored by st(i, v), eight loads per thread in flight per pass (the LDS staging of the
// dVh launches)
template <class Ld, class St>
__device__ __forceinline__ void stage8(int n, Ld ld, St st) {
  for (int i0 = threadIdx.x; i0 < n; i0 += 8 * 256) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = i0 + q * 256;
      v[q] = i < n ? ld(i) : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = i0 + q * 256;
      if (i < n) st(i, v[q]);
    }
  }
}
// n4 float4 of chunk rows from global memory into LDS, eight loads per thread in flight per pass
__device__ __forceinline__ void stage_rows4(float4* dst, const float4* src, int n4) {
  int i = threadIdx.x;
  for (; i + 7 * 256 < n4; i += 8 * 256) {
    float4 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = src[i + q * 256];
#pragma unroll
    for (int q = 0; q < 8; ++q) dst[i + q * 256] = v[q];
  }
  for (; i < n4; i += 256) dst[i] = src[i];
}

constexpr int kXStampSlots = 16;  // per (workgroup, step): phase ends 0..7, sub-phases 8..15
#define XSTAMP(ph)                                                                                 \
  do {                                                                                             \
    if (k.stamps && tid == 0)                                                                      \
      k.stamps[((long)(cs.chain * kXWG + w) * T + t) * kXStampSlots + (ph)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)

// prologue marks of the launch (slots 11-15 of the first processed step t0): 15 entry, 13 sentinel slots re-armed,
// 12 chain census done, 11 chunk rows staged, 14 the step loop starts (tools/xdec_stamps.py)
#define XSTAMP_PRO(t0, ph)                                                                         \
  do {                                                                                             \
    if (k.stamps && tid == 0)                                                                      \
      k.stamps[((long)(cs.chain * kXWG + w) * T + (t0)) * kXStampSlots + (ph)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)

// chain-local operand row of this lane: utterance b0 + min(lane & 15, nU - 1)
__device__ __forceinline__ int xrow(int b0, int nU, int lane) { return b0 + min(lane & 15, nU - 1); }

template <int S, int A, int SC>
__host__ __device__ constexpr size_t xdec_lds(int xlc, int res = 2) {
  return res == 2 ? sizeof(float) * (size_t)xlc * (A + SC) : res == 1 ? sizeof(float) * (size_t)xlc * SC : 0;
}

// F3's wait for the chunk partials of one utterance: every lane loads its column's NC partial
// contexts (chunks past NCH re-read chunk NCH - 1, so all loads of a pass are in flight together),
// lanes j < NCH chunk j's max and lanes 32 + j its sum; each wave polls on its own.
template <int NC>
__device__ __forceinline__ bool poll_combine(const granule_t* PM, const granule_t* PL, const granule_t* PC, int NCH,
                                             int A, int a, bool col, unsigned tag, int lane, float (&pc)[kXMaxCh],
                                             float& pml, unsigned* abort_word) {
  const bool lm = lane < NCH, ll = lane >= 32 && lane - 32 < NCH;
  const granule_t* gml = lm ? PM + lane : ll ? PL + (lane - 32) : PM;
  unsigned spins = 0;
  while (true) {
    const granule_t g = __hip_atomic_load(gml, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool ok = !(lm || ll) || (unsigned)(g >> 32) == tag;
    pml = __uint_as_float((unsigned)g);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int jj = j < NCH ? j : NCH - 1;
      const granule_t xc =
          col ? __hip_atomic_load(PC + (long)jj * A + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ((granule_t)tag << 32);
      ok = ok && (unsigned)(xc >> 32) == tag;
      pc[j] = __uint_as_float((unsigned)xc);
    }
    if (__all(ok)) return true;
    if (spin_give_up(spins, abort_word)) return false;
  }
}

// B45's wait for one column of an utterance's chunk partials (chunks past NCH re-read chunk NCH - 1,
// so all loads of a pass are in flight together)
template <int NC>
__device__ __forceinline__ bool poll_column(const granule_t* P, int NCH, int ld, int j, unsigned tag,
                                            float (&v)[kXMaxCh], unsigned* abort_word) {
  unsigned spins = 0;
  while (true) {
    bool ok = true;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const int qq = q < NCH ? q : NCH - 1;
      const granule_t g = __hip_atomic_load(P + (long)qq * ld + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ok = ok && (unsigned)(g >> 32) == tag;
      v[q] = __uint_as_float((unsigned)g);
    }
    if (ok) return true;
    if (spin_give_up(spins, abort_word)) return false;
  }
}

// ------------------------------------------------------------------------------ forward
template <int S, int A, int SC, int RES, bool R4>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dec_xcd_fwd(AttnK k, XArgs x) {
  constexpr int NS = S / 64, NA = A / 64, NV = (SC / 4 + 63) / 64;
  __shared__ SkinnyRed red;
  // RES = 2: the chunk's h and Vh rows are staged in LDS for the launch (chunks up to kXLC frames);
  // RES = 1: only the Vh rows (the tanh operand) are staged, h rows are read from global memory (L2)
  // every step; RES = 0: both are read every step.  (Longer utterances: chunks up to kXLCStream frames.)
  constexpr int XM = RES == 2 ? kXLC : kXLCStream;
  __shared__ float scs[XM];  // XM = the largest chunk
  __shared__ __attribute__((aligned(16))) float sprev[16][16];
  __shared__ int abort_lds, local_lds, wide_lds;
  __shared__ unsigned tb_lds;
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];  // h rows [kXLC][A] | Vh rows [kXLC][SC]
  const ChainSlot cs = chain_slot(kXWG);
  if (cs.chain >= x.nchains) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w = cs.member;
  const int B = k.B, T = k.T, L = k.L, NCH = x.NCH, XLC = x.XLC, FPW = XLC / 4;
  const int b0 = cs.chain * x.U, nU = min(x.U, B - b0);
  XSTAMP_PRO(0, 15);
  // R4 (chains of <= 4 utterances, handoff.h mfma4_aw_acc): operand rows dealt by lane & 3.  The sentinel slots the
  // skinny products sweep are chain-interleaved (rearm_ilv): a k-quad of the chain's rows is one 16 nU-byte run, so
  // each quad of lanes reads one line (in [B][W] rows: 4 lines per quad)
  const int rr = R4 ? min(lane & 3, nU - 1) : min(lane & 15, nU - 1), br = b0 + rr;
  const int km = nU;
  auto soff = [&](long step_base, long W) -> long { return 4 * (step_base + (long)b0 * W + 4 * rr); };
  auto sidx = [&](long W, int b, int n) -> long { return (long)b0 * W + (long)(n >> 2) * 4 * nU + 4 * (b - b0) + (n & 3); };
  const int orow = tid >> 4, oj = tid & 15;  // this thread's skinny output (row in chain, column in tile)
  const int ob = b0 + orow;
  const bool live = orow < nU;
  unsigned* abort_word = reinterpret_cast<unsigned*>(k.fhdr);
  if (tid == 0) {
    abort_lds = 0;
    wide_lds = g_dec_pf ? 0 : 1;
  }
  const unsigned tb = launch_tagbase(abort_word, &tb_lds);
  const long sS = (long)B * S, sSc = (long)B * SC, sA = (long)B * A;

  // roles
  const bool f1ws = w < SC / 16, f1us = w < 2 * S / 16, f1 = f1ws || f1us;
  const bool zw = w < S / 16, rw = w >= S / 16 && w < 2 * S / 16;
  const int ntask = nU * NCH;
  const bool att = w < ntask;
  const int ub = b0 + (att ? w / NCH : 0), ch = att ? w % NCH : 0;
  const int Lub = frames_of(k, ub);  // frames of this workgroup's utterance (variable-length batch), read once
  const int ncg = (A + 255) / 256;
  const bool f3 = w < nU * ncg;
  // sentinel slots this workgroup publishes (s_t: z tiles, q_t: r tiles, c_t: combine columns)
  if (zw) rearm_ilv(x.sS, sS, T, S, b0, nU, 0, nU, w * 16, 16);
  if (f1ws) rearm_rect(x.sWS, sSc, T, SC, b0, nU, w * 16, 16);  // ws_t: read as utterance rows by F2
  if (rw) rearm_ilv(x.sQ, sS, T, S, b0, nU, 0, nU, (w - S / 16) * 16, 16);
  if (f3) rearm_ilv(x.sC, sA, T, A, b0, nU, w / ncg, 1, 256 * (w % ncg), min(256, A - 256 * (w % ncg)));
  rearm_done();
  XSTAMP_PRO(0, 13);
  const bool loc = chain_is_local(x.fcensus, cs.chain, kXWG, w, x.allow_local != 0, abort_word, &local_lds, tb);
  XSTAMP_PRO(0, 12);
  // r tiles: s_{t-1} of units [jt, jt + 16) is chunk it of wave wt in the F1 sweep
  const int jt = (w - S / 16) * 16, wt = (jt % 64) / 16, it = jt / 64;

  float4 wws[NS], wus[NS], wg0[NA], wg1[NA], whs[NS];
  if (f1ws) load_wfrag(wws, k.P.Ws + (long)(w * 16 + (lane & 15)) * S, wave, lane);
  if (f1us) {
    const float* Wg = zw ? k.P.Wz + (long)(w * 16 + (lane & 15)) * 2 * S
                         : k.P.Wr + (long)((w - S / 16) * 16 + (lane & 15)) * 2 * S;
    load_wfrag(wus, Wg, wave, lane);
  }
  if (zw) {
    load_wfrag(wg0, x.WX + (long)(w * 16 + (lane & 15)) * A, wave, lane);              // gx_z tile
    load_wfrag(wg1, x.WX + (long)(2 * S + w * 16 + (lane & 15)) * A, wave, lane);      // gx_h tile
    load_wfrag(whs, k.P.Wh + (long)(w * 16 + (lane & 15)) * 2 * S, wave, lane);        // Wh_s tile
  } else if (rw) {
    load_wfrag(wg0, x.WX + (long)(S + (w - S / 16) * 16 + (lane & 15)) * A, wave, lane);  // gx_r tile
  }
  const float* hres = RES == 2 ? dyn_lds : k.h + ((long)ub * L + ch * XLC) * A;
  const float* vres = RES == 2 ? dyn_lds + XLC * A : RES == 1 ? dyn_lds : k.Vh + ((long)ub * L + ch * XLC) * SC;
  bool pf = false;  // product-form attention terms (stage_vh): vres holds E = 2^(K Vh) (RES > 0)
  if (att) {
    const int rows = min(XLC, L - ch * XLC);
    const int n4h = rows * A / 4, n4v = rows * SC / 4;
    const float4* hs = reinterpret_cast<const float4*>(k.h + ((long)ub * L + ch * XLC) * A);
    const float4* vs = reinterpret_cast<const float4*>(k.Vh + ((long)ub * L + ch * XLC) * SC);
    if (RES == 2)
      stage_rows4(reinterpret_cast<float4*>(dyn_lds), hs, n4h);
    pf = stage_vh<RES>(reinterpret_cast<float4*>(dyn_lds + (RES == 2 ? XLC * A : 0)), vs, n4v, &wide_lds);
  }
  __syncthreads();
  XSTAMP_PRO(0, 11);

  // step-invariant operands in registers: we (attention), bs (ws tile)
  float4 wev[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c4 = lane + 64 * j;
    wev[j] = c4 < SC / 4 ? reinterpret_cast<const float4*>(k.P.we)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float bsn = f1ws ? k.P.bs[w * 16 + oj] : 0.f;
  float esum = 0.f;  // sum_j we_j (tanh_r)
#pragma unroll
  for (int j = 0; j < NV; ++j) esum += (wev[j].x + wev[j].y) + (wev[j].z + wev[j].w);
  esum = wave_sum_dpp(esum);
  float zreg = 0.f, gxh = 0.f, sreg = 0.f;
  float4 cav[NA];  // c_t's operand chunks, swept in F4 and kept for F5's Wx'_h c
  float4 sav[NS];  // s_{t-1}'s operand chunks, swept in F1 and kept for F4's us half
  XSTAMP_PRO(0, 14);
  for (int t = 0; t < T; ++t) {
    const unsigned tag = tb + t + 1;
    const long sl = t & 1, slp = (t - 1) & 1;
    const long row = (long)ob * T + t;
    XSTAMP(0);
    // ---- F1: ws = Ws s_{t-1} + bs  (s_{t-1}'s chunks kept for F4's us = [Wz_s; Wr_s] s_{t-1})
    if (f1) {
      floatx4 a1 = {0.f, 0.f, 0.f, 0.f};
      bool ok = true;
      float4 (&av)[NS] = sav;  // s_{t-1}'s operand chunks, kept for F4's us half
      if (t > 0) {
        ok = loc ? sweep_sent<NS>(av, rsrc_of(x.sS), soff((t - 1) * sS, S), wave, lane, abort_word, km)
                 : sweep_skinny<NS>(av, rsrc_of(x.gS), 8 * (slp * sS + (long)br * S), tb + t, wave, lane, abort_word);
        if (f1ws) a1 = mfma_rows_aw<R4, NS>(av, wws, lane);
        if (rw && wave == wt) {
#pragma unroll
          for (int i = 0; i < NS; ++i)
            if (i == it) *reinterpret_cast<float4*>(&sprev[lane & 15][4 * (lane >> 4)]) = av[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) av[i] = make_float4(0.f, 0.f, 0.f, 0.f);  // s_{-1} = 0
      }
      float v1;
      const bool f1ok = dec_sync(red, &abort_lds, ok, a1, wave, lane, tid, &v1);
      if (f1ws) {
        const int n = w * 16 + oj;
        const float v = v1 + bsn;
        if (loc) {  // sentinel rows (4 bytes a value) on a local chain, tagged granules otherwise
          if (live) put_sent(x.sWS + t * sSc + (long)ob * SC + n, v);
        } else {
          put_granule_pair(x.gWS, sl * sSc + (long)ob * SC + n, v, tag, live);
        }
        if (live) k.WS[row * SC + n] = v;
      }
      // (us = [Wz_s; Wr_s] s_{t-1} is F4's first half now: multiplied while c is in flight, one reduce with gx)
      if (!f1ok) return;  // abort checked after the phase: its LDS read is issued with the reduce's
    }
    XSTAMP(1);
    // ---- F2: attention chunk (ub, ch): scores, local softmax stats, partial context
    if (att) {
      float4 wsv[NV];
      bool ok = loc ? sweep_vec_sent<NV>(wsv, rsrc_of(x.sWS), 4 * (t * sSc + (long)ub * SC), SC / 4, lane, abort_word)
                    : sweep_vec<NV>(wsv, rsrc_of(x.gWS), 8 * (sl * sSc + (long)ub * SC), SC / 4, tag, lane, abort_word);
      XSTAMP(6);  // sub-phase: ws_t arrived
      const int Lu = Lub;  // frames of this utterance (variable-length batch)
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        wsv[j].x *= kTanhK; wsv[j].y *= kTanhK; wsv[j].z *= kTanhK; wsv[j].w *= kTanhK;
        if (lane + 64 * j >= SC / 4) wsv[j] = make_float4(0.f, 0.f, 0.f, 0.f);  // (not swept: finite for the terms)
      }
      // the wave's frames in groups of four: the four frames' Vh loads issued together, their 4 NV x 4 terms as
      // independent chains, then four DPP reductions.  Branch-free: a frame past the wave's share or past the
      // utterance reads a valid row of the chunk and its sum is dropped by a select afterwards (per-frame branches
      // serialised the frames -- one load wait and one dependent exp / rcp chain after the other, ~0.25 us a frame).
      // score = esum - 2 sum_j we_j r_j
      const int lmax = min(XLC, L - ch * XLC) - 1;  // last row of the chunk
      // product form (pf, uniform): W_j = 2^(K ws_j) once per column, r = 1 / (E W + 1)
      float4 wex[NV];
      if (pf) {
#pragma unroll
        for (int j = 0; j < NV; ++j)
          wex[j] = make_float4(__builtin_amdgcn_exp2f(wsv[j].x), __builtin_amdgcn_exp2f(wsv[j].y),
                               __builtin_amdgcn_exp2f(wsv[j].z), __builtin_amdgcn_exp2f(wsv[j].w));
      }
      auto scores = [&](auto pfc) {
        constexpr bool PF = decltype(pfc)::value;
#pragma unroll
        for (int i0 = 0; i0 < XM / 4; i0 += 4) {
          if (i0 >= FPW) break;
          float4 vv[4][NV];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int li = min(wave * FPW + min(i0 + u, FPW - 1), lmax);
            const float4* vh4 = reinterpret_cast<const float4*>(vres + (long)li * SC);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              const int c4 = lane + 64 * j;
              vv[u][j] = c4 < SC / 4 ? vh4[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
              if (PF && RES == 0) vv[u][j] = pf_e4(vv[u][j]);  // (the staged levels hold E already)
            }
          }
          float part[4];
          // (components in packed pairs: .x the x / z terms, .y the y / w terms -- the two sums s0, s1 of the scalar
          // form, bitwise)
          const floatx2 one2 = {1.f, 1.f}, k2 = {kTanhK, kTanhK};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            floatx2 s2 = {0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              const float4 v = vv[u][j];
              const float4 e = wev[j];  // (0 on columns past SC: the term drops out)
              if (PF) {
                const float4 wx = wex[j];
                s2 = pk_fma(floatx2{e.x, e.y}, rcp2(pk_fma(floatx2{v.x, v.y}, floatx2{wx.x, wx.y}, one2)), s2);
                s2 = pk_fma(floatx2{e.z, e.w}, rcp2(pk_fma(floatx2{v.z, v.w}, floatx2{wx.z, wx.w}, one2)), s2);
              } else {
                const float4 ww = wsv[j];
                const floatx2 za = pk_fma(floatx2{v.x, v.y}, k2, floatx2{ww.x, ww.y});
                const floatx2 zb = pk_fma(floatx2{v.z, v.w}, k2, floatx2{ww.z, ww.w});
                s2 = pk_fma(floatx2{e.x, e.y}, floatx2{tanh_r(za.x), tanh_r(za.y)}, s2);
                s2 = pk_fma(floatx2{e.z, e.w}, floatx2{tanh_r(zb.x), tanh_r(zb.y)}, s2);
              }
            }
            const int l = ch * XLC + wave * FPW + i0 + u;
            part[u] = (i0 + u < FPW && l < Lu) ? s2.x + s2.y : 0.f;
          }
          // the four frames' wave sums in one transposed reduction: lanes 0-3 hold them (wave_sum4_slot)
          const float tot = wave_sum4_t(part[0], part[1], part[2], part[3], lane);
          if (lane < 4) {
            const int u = wave_sum4_slot(lane), li = wave * (FPW) + i0 + u, l = ch * XLC + li;
            if (i0 + u < FPW) scs[li] = l < Lu ? fmaf(-2.f, tot, esum) : -INFINITY;
          }
        }
      };
      if (pf) scores(std::true_type{});
      else scores(std::false_type{});
      XSTAMP(7);  // sub-phase: this wave's scores done
      if (!ok) abort_lds = 1;
      __syncthreads();  // scs complete
      const bool f2ok = abort_lds == 0;
      // the chunk's softmax statistics in every wave (DPP reductions, no further barrier): lane i
      // holds frame i's score and its weight p_i = exp(e_i - m)
      const int lend = min(XLC, L - ch * XLC);
      const float sv = lane < XLC ? scs[lane] : -INFINITY;
      const float m = wave_max_dpp(sv);
      const float p = (lane < XLC && ch * XLC + lane < Lu) ? expf(sv - m) : 0.f;
      const float psum = wave_sum_dpp(p);
      if (wave == 0) {
        const int l = ch * XLC + lane;
        if (lane < XLC && l < L) k.E[((long)ub * T + t) * L + l] = sv;
        if (lane == 0) {
          put_granule(x.gPM + sl * B * NCH + (long)ub * NCH + ch, m, tag, loc);
          put_granule(x.gPL + sl * B * NCH + (long)ub * NCH + ch, psum, tag, loc);
        }
      }
      // partial context: two adjacent columns per thread, frame weights broadcast from lane i
      const long pcoff = sl * (long)B * NCH * A + ((long)ub * NCH + ch) * A;
      for (int a2 = tid; a2 < A / 2; a2 += 256) {
        float2 acc = {0.f, 0.f};
        int i = 0;
        // eight frames' h loads in flight before their (in-order) accumulation: one load round trip per eight
        // frames instead of per frame
        for (; i + 8 <= lend; i += 8) {
          float2 hv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) hv[u] = reinterpret_cast<const float2*>(hres + (long)(i + u) * A)[a2];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const float pi = lane_f32(p, i + u);
            acc.x += pi * hv[u].x;
            acc.y += pi * hv[u].y;
          }
        }
        for (; i < lend; ++i) {
          const float2 hv = reinterpret_cast<const float2*>(hres + (long)i * A)[a2];
          const float pi = lane_f32(p, i);
          acc.x += pi * hv.x;
          acc.y += pi * hv.y;
        }
        put_granule2(rsrc_of(x.gPC), 8 * (pcoff + 2L * a2), acc.x, acc.y, tag, loc);
      }
      __syncthreads();  // scs is rewritten next step
      if (!f2ok) return;
    }
    XSTAMP(2);
    // ---- F3: combine the chunks of utterance cb for columns [a0, a0 + 256) -> c, lse
    if (f3) {
      const int cb = b0 + w / ncg, a = 256 * (w % ncg) + tid;
      const bool col = a < A;
      const granule_t* PM = x.gPM + sl * B * NCH + (long)cb * NCH;
      const granule_t* PL = x.gPL + sl * B * NCH + (long)cb * NCH;
      const granule_t* PC = x.gPC + sl * (long)B * NCH * A + (long)cb * NCH * A;
      float pc[kXMaxCh];
      float pml = 0.f;  // lane j < NCH: chunk j's max; lane 32 + j: its sum
      const bool ok = NCH <= 8 ? poll_combine<8>(PM, PL, PC, NCH, A, a, col, tag, lane, pc, pml, abort_word)
                               : poll_combine<kXMaxCh>(PM, PL, PC, NCH, A, a, col, tag, lane, pc, pml, abort_word);
      // chunk weights e_j = exp(m_j - m) once per lane, broadcast with v_readlane
      const float mj = lane < NCH ? pml : -INFINITY;
      const float m = wave_max_dpp(mj);
      const float ej = lane < NCH ? expf(pml - m) : 0.f;
      const float lj = __shfl(pml, (lane + 32) & 63, 64);  // chunk lane's sum
      const float den = wave_sum_dpp(ej * (lane < NCH ? lj : 0.f));
      float acc = 0.f;
      for (int j = 0; j < NCH; ++j) acc += lane_f32(ej, j) * pc[j];
      const long crow = (long)cb * T + t;
      if (tid == 0 && a == 0) k.LSE[crow] = m + logf(den);
      const float c = acc * (1.0f / den);
      if (loc) {
        if (col && ok) put_sent(x.sC + t * sA + sidx(A, cb, a), c);
      } else {
        put_granule_pair(x.gC, sl * sA + (long)cb * A + a, c, tag, col && ok);
      }
      if (col && ok) {
        k.C[crow * A + a] = c;
        k.VV[crow * (S + A) + S + a] = c;
      }
      if (!ok) abort_lds = 1;  // no LDS data crosses waves in F3: agreed on at F4's reduce
    }
    XSTAMP(3);
    // ---- F4: z = sig([Wz_s | Wx'_z] [s_{t-1}; c] + KX_z), r likewise, q = r s_{t-1}
    if (zw || rw) {
      // teacher-forced gate constants of this step (no dependence on the hand-off): load first
      const float* kx = x.KX + row * 3 * S;
      const float kx0 = live ? (zw ? kx[w * 16 + oj] : kx[S + (w - S / 16) * 16 + oj]) : 0.f;
      const float kx1 = (live && zw) ? kx[2 * S + w * 16 + oj] : 0.f;
      // one product over [s_{t-1}; c] (K = S + A): the us half (s_{t-1} swept in F1) runs while c is in flight
      bool ok = true;
      floatx4 acc0, acc1;
      if (loc) {
        uint4 craw[NA];
        sent_row_issue<NA>(craw, rsrc_of(x.sC), soff(t * sA, A), wave, lane, km);
        __builtin_amdgcn_sched_barrier(0);  // the c loads stay ahead of the us-half MFMAs
        mfma_rows_acc<R4, NS>(sav, wus, acc0, acc1, true);
        __builtin_amdgcn_sched_barrier(0);
        if (!sent_tile_check<NA>(craw, cav))
          ok = sweep_sent<NA>(cav, rsrc_of(x.sC), soff(t * sA, A), wave, lane, abort_word, km);
      } else {
        ok = sweep_skinny<NA>(cav, rsrc_of(x.gC), 8 * (sl * sA + (long)br * A), tag, wave, lane, abort_word);
        mfma_rows_acc<R4, NS>(sav, wus, acc0, acc1, true);
      }
      mfma_rows_acc<R4, NA>(cav, wg0, acc0, acc1, false);
      const floatx4 a1 = mfma_rows_done<R4>(acc0, acc1, lane);
      float g0;
      const bool f4ok = dec_sync(red, &abort_lds, ok, a1, wave, lane, tid, &g0);
      if (zw) {  // (gx_h = Wx'_h c runs in F5, beside the q hand-off, on the c kept in cav)
        const int n = w * 16 + oj;
        zreg = sigmoidf_(g0 + kx0);
        gxh = kx1;
        if (live) k.GSV[row * 3 * S + n] = zreg;
      } else {
        const int j = (w - S / 16) * 16 + oj;
        const float r = sigmoidf_(g0 + kx0);
        const float sp = t > 0 ? sprev[orow][oj] : 0.f;
        const float q = r * sp;
        if (loc) {
          if (live) put_sent(x.sQ + t * sS + sidx(S, ob, j), q);
        } else {
          put_granule_pair(x.gQ, sl * sS + (long)ob * S + j, q, tag, live);
        }
        if (live) {
          k.GSV[row * 3 * S + S + j] = r;
          k.RHX[row * 2 * S + j] = q;
        }
      }
      if (!f4ok) return;
    }
    XSTAMP(4);
    // ---- F5: hh = tanh(Wx'_h c + Wh_s q + KX_h); s_t = (1-z) s_{t-1} + z hh -- one product over the concatenated
    // K = A + S (one cross-wave reduce): the q tile is loaded first, the c half (c from F4, already in registers)
    // multiplied while q is in flight, then q is checked (polled further only if not yet published)
    if (zw) {
      float4 aq[NS];
      bool ok = true;
      floatx4 acc0, acc1;
      if (loc) {
        uint4 qraw[NS];
        sent_row_issue<NS>(qraw, rsrc_of(x.sQ), soff(t * sS, S), wave, lane, km);
        __builtin_amdgcn_sched_barrier(0);  // the q loads stay ahead of the c-half MFMAs
        mfma_rows_acc<R4, NA>(cav, wg1, acc0, acc1, true);
        __builtin_amdgcn_sched_barrier(0);
        if (!sent_tile_check<NS>(qraw, aq))
          ok = sweep_sent<NS>(aq, rsrc_of(x.sQ), soff(t * sS, S), wave, lane, abort_word, km);
      } else {
        ok = sweep_skinny<NS>(aq, rsrc_of(x.gQ), 8 * (sl * sS + (long)br * S), tag, wave, lane, abort_word);
        mfma_rows_acc<R4, NA>(cav, wg1, acc0, acc1, true);
      }
      mfma_rows_acc<R4, NS>(aq, whs, acc0, acc1, false);
      const floatx4 a1 = mfma_rows_done<R4>(acc0, acc1, lane);
      float v;
      const bool f5ok = dec_sync(red, &abort_lds, ok, a1, wave, lane, tid, &v);
      const int n = w * 16 + oj;
      const float hh = tanhf(v + gxh);
      const float z = zreg, sp = sreg;
      sreg = (-z + 1.0f) * sp + z * hh;
      if (loc) {
        if (live) put_sent(x.sS + t * sS + sidx(S, ob, n), sreg);
      } else {
        put_granule_pair(x.gS, sl * sS + (long)ob * S + n, sreg, tag, live);
      }
      if (live) {
        k.GSV[row * 3 * S + 2 * S + n] = hh;
        k.VV[row * (S + A) + n] = sreg;
        if (t + 1 < T) {
          k.HX[(row + 1) * 2 * S + n] = sreg;
        }
      }
      if (!f5ok) return;
    }
    XSTAMP(5);
  }
}

// ------------------------------------------------------------------------------ backward
template <int S, int A, int SC, int RES, bool R4>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dec_xcd_bwd(AttnK k, XArgs x) {
  constexpr int NS = S / 64, NSC = SC / 64, NG = 3 * S / 64;
  constexpr int NVA = (A / 4 + 63) / 64;
  __shared__ SkinnyRed red, red2;
  __shared__ float redv[4];
  __shared__ __attribute__((aligned(16))) float dcs[A];
  __shared__ __attribute__((aligned(16))) float cs_[A];
  constexpr int XM = RES == 2 ? kXLC : kXLCStream;
  __shared__ __attribute__((aligned(16))) float des[XM];  // XM = the largest chunk
  __shared__ int abort_lds, local_lds, wide_lds;
  __shared__ unsigned tb_lds;
  extern __shared__ __attribute__((aligned(16))) float dyn_lds[];  // h rows [kXLC][A] | Vh rows [kXLC][SC]
  const ChainSlot cs = chain_slot(kXWG);
  if (cs.chain >= x.nchains) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w = cs.member;
  const int B = k.B, T = k.T, L = k.L, NCH = x.NCH, XLC = x.XLC, FPW = XLC / 4;
  const int b0 = cs.chain * x.U, nU = min(x.U, B - b0);
  XSTAMP_PRO(T - 1, 15);
  // R4 (chains of <= 4 utterances, handoff.h mfma4_aw_acc): operand rows dealt by lane & 3.  The sentinel slots the
  // skinny products sweep are chain-interleaved (rearm_ilv): a k-quad of the chain's rows is one 16 nU-byte run, so
  // each quad of lanes reads one line (in [B][W] rows: 4 lines per quad)
  const int rr = R4 ? min(lane & 3, nU - 1) : min(lane & 15, nU - 1), br = b0 + rr;
  const int km = nU;
  auto soff = [&](long step_base, long W) -> long { return 4 * (step_base + (long)b0 * W + 4 * rr); };
  auto sidx = [&](long W, int b, int n) -> long { return (long)b0 * W + (long)(n >> 2) * 4 * nU + 4 * (b - b0) + (n & 3); };
  const int orow = tid >> 4, oj = tid & 15;
  const int ob = b0 + orow;
  const bool live = orow < nU;
  unsigned* abort_word = reinterpret_cast<unsigned*>(k.bhdr);
  if (tid == 0) {
    abort_lds = 0;
    wide_lds = g_dec_pf ? 0 : 1;
  }
  const unsigned tb = launch_tagbase(abort_word, &tb_lds);
  const long sS = (long)B * S, sSc = (long)B * SC, sA = (long)B * A;

  const bool sw = w < S / 16;     // S-tile: gate grads, dq, us', ds for units [16w, 16w + 16)
  const bool dcw = w < A / 16;    // dc tile
  const int ntask = nU * NCH;
  const bool att = w < ntask;
  const int ub = b0 + (att ? w / NCH : 0), ch = att ? w % NCH : 0;
  const int Lub = frames_of(k, ub);  // frames of this workgroup's utterance (variable-length batch), read once
  const int nsg = (SC + 255) / 256;
  const bool rdw = w < nU * nsg;  // dws reduction (utterance, 256 columns)
  const int n = w * 16 + oj;      // S-tile unit of this thread
  // sentinel slots this workgroup publishes
  if (sw) {
    rearm_ilv(x.sDGZ, sS, T, S, b0, nU, 0, nU, w * 16, 16);
    rearm_ilv(x.sDGR, sS, T, S, b0, nU, 0, nU, w * 16, 16);
    rearm_ilv(x.sDGH, sS, T, S, b0, nU, 0, nU, w * 16, 16);
  }
  if (dcw) rearm_rect(x.sDC, sA, T, A, b0, nU, w * 16, 16);  // (dc: read as utterance rows by B4, not interleaved)
  if (rdw) rearm_ilv(x.sDWS, sSc, T, SC, b0, nU, w / nsg, 1, 256 * (w % nsg), min(256, SC - 256 * (w % nsg)));
  rearm_done();
  XSTAMP_PRO(T - 1, 13);
  const bool loc = chain_is_local(x.bcensus, cs.chain, kXWG, w, x.allow_local != 0, abort_word, &local_lds, tb);
  XSTAMP_PRO(T - 1, 12);

  float4 wq[NS], wus[2 * NS], wdc[NG], wsT[NSC];
  if (sw) {
    load_wfrag(wq, x.XWHT + (long)(w * 16 + (lane & 15)) * S, wave, lane);
    load_wfrag(wus, x.XZRT + (long)(w * 16 + (lane & 15)) * 2 * S, wave, lane);
    load_wfrag(wsT, x.XWST + (long)(w * 16 + (lane & 15)) * SC, wave, lane);
  }
  if (dcw) load_wfrag(wdc, x.WXT + (long)(w * 16 + (lane & 15)) * 3 * S, wave, lane);
  const float* hres = RES == 2 ? dyn_lds : k.h + ((long)ub * L + ch * XLC) * A;
  const float* vres = RES == 2 ? dyn_lds + XLC * A : RES == 1 ? dyn_lds : k.Vh + ((long)ub * L + ch * XLC) * SC;
  bool pf = false;  // product-form attention terms (stage_vh): vres holds E = 2^(K Vh) (RES > 0)
  if (att) {
    const int rows = min(XLC, L - ch * XLC);
    const int n4h = rows * A / 4, n4v = rows * SC / 4;
    const float4* hs = reinterpret_cast<const float4*>(k.h + ((long)ub * L + ch * XLC) * A);
    const float4* vs = reinterpret_cast<const float4*>(k.Vh + ((long)ub * L + ch * XLC) * SC);
    if (RES == 2)
      stage_rows4(reinterpret_cast<float4*>(dyn_lds), hs, n4h);
    pf = stage_vh<RES>(reinterpret_cast<float4*>(dyn_lds + (RES == 2 ? XLC * A : 0)), vs, n4v, &wide_lds);
  }
  __syncthreads();
  XSTAMP_PRO(T - 1, 11);

  // ds_t of this thread's (utterance, unit); gate-grad inputs of step t
  // forward activations of step t for this thread's (utterance, unit), loaded one step ahead (during
  // B5's wait) so the gate gradients that open each step read registers only
  struct Act {
    float z, r, hh, sp, dv;
  };
  auto load_act = [&](int t) {
    Act a{0.f, 0.f, 0.f, 0.f, 0.f};
    if (sw && live) {
      const long row = (long)ob * T + t;
      a.z = k.GSV[row * 3 * S + n]; a.r = k.GSV[row * 3 * S + S + n]; a.hh = k.GSV[row * 3 * S + 2 * S + n];
      a.sp = k.HX[row * 2 * S + n];
      a.dv = k.DV[row * (S + A) + n];
    }
    return a;
  };
  Act cur = load_act(T - 1);
  float ds = cur.dv, dsp = 0.f, usp = 0.f;
  XSTAMP_PRO(T - 1, 14);
  for (int p = 0; p < T; ++p) {
    const int t = T - 1 - p;
    const unsigned tag = tb + p + 1;
    const long sl = p & 1;
    const long row = (long)ob * T + t;
    XSTAMP(0);
    const float z = cur.z, r = cur.r, sp = cur.sp;
    // ---- G: gate grads of step t (da_h first: it gates B2)
    if (sw) {
      const float hh = cur.hh;
      const float daz = ds * (hh - sp) * (z * (1.0f - z));
      const float dah = (ds * z) * (1.0f - hh * hh);
      if (loc) {
        if (live) {
          put_sent(x.sDGH + p * sS + sidx(S, ob, n), dah);
          put_sent(x.sDGZ + p * sS + sidx(S, ob, n), daz);
        }
      } else {
        put_granule_pair(x.gDGH, sl * sS + (long)ob * S + n, dah, tag, live);
        put_granule_pair(x.gDGZ, sl * sS + (long)ob * S + n, daz, tag, live);
      }
      if (live) {
        k.DGA[row * 3 * S + n] = daz;
        k.DGA[row * 3 * S + 2 * S + n] = dah;
      }
    }
    XSTAMP(1);
    // ---- B2: dq = Wh_s^T da_h -> da_r; dsp = ds (1-z) + dq r
    float4 bh[NS];  // da_h operand of B2's sweep (B3's h chunks in S-tile workgroups)
    if (sw) {
      float4 (&av)[NS] = bh;
      const bool ok =
          loc ? sweep_sent<NS>(av, rsrc_of(x.sDGH), soff(p * sS, S), wave, lane, abort_word, km)
              : sweep_skinny<NS>(av, rsrc_of(x.gDGH), 8 * (sl * sS + (long)br * S), tag, wave, lane, abort_word);
      const floatx4 a1 = mfma_rows_aw<R4, NS>(av, wq, lane);
      float dq;
      const bool b2ok = dec_sync(red, &abort_lds, ok, a1, wave, lane, tid, &dq);
      const float dar = (dq * sp) * (r * (1.0f - r));
      if (loc) {
        if (live) put_sent(x.sDGR + p * sS + sidx(S, ob, n), dar);
      } else {
        put_granule_pair(x.gDGR, sl * sS + (long)ob * S + n, dar, tag, live);
      }
      if (live) k.DGA[row * 3 * S + S + n] = dar;
      dsp = ds * (-z + 1.0f) + dq * r;
      if (!b2ok) return;
    }
    XSTAMP(2);
    // ---- B3: dc = Wx'^T [da_z; da_h; da_r] + dc_mlp ; us' = [Wz_s; Wr_s]^T [da_z; da_r]
    // da_z and da_h were published in G: their chunks are swept and multiplied first (in the dc-only workgroups while
    // the S-tile workgroups run B2), so only da_r's chunks wait on B2's hand-off
    if (dcw || sw) {
      const float dcm = (dcw && live) ? k.DV[row * (S + A) + S + w * 16 + oj] : 0.f;  // dc_mlp, hand-off free
      float4 az[NS], ah[NS], ar[NS];
      if (sw) {
#pragma unroll
        for (int i = 0; i < NS; ++i) ah[i] = bh[i];
      }
      {
        bool ok;
        if (sw) {  // (S-tile workgroups hold da_h from B2)
          float4 ag[1][NS];
          if (loc) {
            const __amdgpu_buffer_rsrc_t rs1[1] = {rsrc_of(x.sDGZ)};
            const long off1[1] = {soff(p * sS, S)};
            ok = sweep_sent_rows<NS, 1>(ag, rs1, off1, wave, lane, abort_word, km);
          } else {
            const __amdgpu_buffer_rsrc_t rs1[1] = {rsrc_of(x.gDGZ)};
            const long off1[1] = {8 * (sl * sS + (long)br * S)};
            const unsigned tag1[1] = {tag};
            ok = sweep_skinny_rows<NS, 1>(ag, rs1, off1, tag1, wave, lane, abort_word);
          }
#pragma unroll
          for (int i = 0; i < NS; ++i) az[i] = ag[0][i];
        } else {
          float4 ag[2][NS];
          if (loc) {
            const __amdgpu_buffer_rsrc_t rs2[2] = {rsrc_of(x.sDGZ), rsrc_of(x.sDGH)};
            const long o = soff(p * sS, S);
            const long off2[2] = {o, o};
            ok = sweep_sent_rows<NS, 2>(ag, rs2, off2, wave, lane, abort_word, km);
          } else {
            const __amdgpu_buffer_rsrc_t rs2[2] = {rsrc_of(x.gDGZ), rsrc_of(x.gDGH)};
            const long o = 8 * (sl * sS + (long)br * S);
            const long off2[2] = {o, o};
            const unsigned tag2[2] = {tag, tag};
            ok = sweep_skinny_rows<NS, 2>(ag, rs2, off2, tag2, wave, lane, abort_word);
          }
#pragma unroll
          for (int i = 0; i < NS; ++i) {
            az[i] = ag[0][i];
            ah[i] = ag[1][i];
          }
        }
        if (!ok) abort_lds = 1;
      }
      float4 wz[NS], wh[NS], wr[NS], uz[NS], ur[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        wz[i] = wdc[i];
        wr[i] = wdc[NS + i];
        wh[i] = wdc[2 * NS + i];
        uz[i] = wus[i];
        ur[i] = wus[NS + i];
      }
      floatx4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0, u0 = c0, u1 = c0;
      if (dcw) {
        mfma_rows_acc<R4, NS>(az, wz, c0, c1, true);
        mfma_rows_acc<R4, NS>(ah, wh, c0, c1, false);
      }
      if (sw) mfma_rows_acc<R4, NS>(az, uz, u0, u1, true);
      {
        bool ok;
        float4 ag[1][NS];
        if (loc) {
          const __amdgpu_buffer_rsrc_t rs1[1] = {rsrc_of(x.sDGR)};
          const long off1[1] = {soff(p * sS, S)};
          ok = sweep_sent_rows<NS, 1>(ag, rs1, off1, wave, lane, abort_word, km);
        } else {
          const __amdgpu_buffer_rsrc_t rs1[1] = {rsrc_of(x.gDGR)};
          const long off1[1] = {8 * (sl * sS + (long)br * S)};
          const unsigned tag1[1] = {tag};
          ok = sweep_skinny_rows<NS, 1>(ag, rs1, off1, tag1, wave, lane, abort_word);
        }
        if (!ok) abort_lds = 1;
#pragma unroll
        for (int i = 0; i < NS; ++i) ar[i] = ag[0][i];
      }
      floatx4 a1 = {0.f, 0.f, 0.f, 0.f};
      if (dcw) {
        mfma_rows_acc<R4, NS>(ar, wr, c0, c1, false);
        a1 = mfma_rows_done<R4>(c0, c1, lane);
      }
      float v1;
      if (!dec_sync(red, &abort_lds, true, a1, wave, lane, tid, &v1)) return;
      if (dcw) {
        const int a = w * 16 + oj;
        const float dc = v1 + dcm;
        if (loc) {
          if (live) put_sent(x.sDC + p * sA + (long)ob * A + a, dc);
        } else {
          put_granule_pair(x.gDC, sl * sA + (long)ob * A + a, dc, tag, live);
        }
        if (live) x.DCS[row * A + a] = dc;
      }
      if (sw) {
        mfma_rows_acc<R4, NS>(ar, ur, u0, u1, false);
        usp = skinny_reduce(red2, mfma_rows_done<R4>(u0, u1, lane), wave, lane, tid);
      }
    }
    XSTAMP(3);
    // ---- B4: attention backward of chunk (ub, ch) at step t -> de (saved), partial dws
    if (att) {
      const long arow = (long)ub * T + t;
      // everything that does not depend on dc is loaded before the dc hand-off (c, the penalty sum, this chunk's
      // alphas, the ws / reference-point columns of the dws sums) and used only after the dc sweep: the sweep's loads
      // then go out right behind them and one wait covers both (used before it, each load waited on its own first)
      const float* alpha = k.ALPHA + arow * L;
      const float lam = k.penalty;
      const float ind = k.IND[arow], indn = t + 1 < T ? k.IND[arow + 1] : 0.f;
      const int Lu = Lub;  // MonotonicAlignment's L for this utterance (alpha = 0 past it)
      constexpr int NCA = (A + 255) / 256;
      float cpre[NCA];
#pragma unroll
      for (int q = 0; q < NCA; ++q) cpre[q] = tid + 256 * q < A ? k.C[arow * A + tid + 256 * q] : 0.f;
      if (lam != 0.f) {  // uniform
        float part = 0.f;
        for (int l = tid; l < L; l += 256) part += alpha[l] * (lam * (float)(Lu - l) * (ind - indn));
        part = wave_sum_dpp(part);
        if (lane == 0) redv[wave] = part;
      } else if (lane == 0) {
        redv[wave] = 0.f;
      }
      float alv[XM / 4];
#pragma unroll
      for (int i = 0; i < XM / 4; ++i) {
        const int l = ch * XLC + wave * FPW + i;
        alv[i] = (i < FPW && l < L) ? alpha[l] : 0.f;
      }
      constexpr int NJ = (SC + 255) / 256;
      float wsj[NJ], ejj[NJ], grf[NJ], vbj[NJ];
      {
        const float* ws = k.WS + arow * SC;
        const float* vbar = x.VBAR + (long)ub * SC;
#pragma unroll
        for (int q = 0; q < NJ; ++q) {
          const int j = tid + 256 * q;
          wsj[q] = j < SC ? ws[j] : 0.f;
          ejj[q] = j < SC ? k.P.we[j] : 0.f;
          vbj[q] = j < SC ? vbar[j] : 0.f;
        }
      }
      {
        float4 dv[NVA];
        const bool ok =
            loc ? sweep_vec_sent<NVA>(dv, rsrc_of(x.sDC), 4 * (p * sA + (long)ub * A), A / 4, lane, abort_word)
                : sweep_vec<NVA>(dv, rsrc_of(x.gDC), 8 * (sl * sA + (long)ub * A), A / 4, tag, lane, abort_word);
        if (wave == 0) {
#pragma unroll
          for (int i = 0; i < NVA; ++i) {
            const int c4 = lane + 64 * i;
            if (c4 < A / 4) reinterpret_cast<float4*>(dcs)[c4] = dv[i];
          }
        }
#pragma unroll
        for (int q = 0; q < NCA; ++q)
          if (tid + 256 * q < A) cs_[tid + 256 * q] = cpre[q];
#pragma unroll
        for (int q = 0; q < NJ; ++q) {
          wsj[q] *= kTanhK;  // K ws (tanh_r)
          // gref_j = g at the utterance's mean Vh row (see the dws sums below), in the terms' own form
          const float rr = tanh_r(fmaf(vbj[q], kTanhK, wsj[q]));
          grf[q] = 4.f * fmaf(-rr, rr, rr);
        }
        if (!ok) abort_lds = 1;
        __syncthreads();  // dcs / cs_ / redv complete
      }
      const bool b4ok = abort_lds == 0;
      XSTAMP(7);  // sub-phase: dc_t arrived
      // softmax backward: de_l = alpha_l (d alpha_l - sum_j alpha_j d alpha_j).  With d alpha_l =
      // h_l . dc + pen_l and sum_j alpha_j h_j = c, the bracket is (h_l - c) . dc + pen_l - sum_j alpha_j
      // pen_j: subtracting c before the dot avoids the cancellation of two 512-term dot products
      const float spen = ((redv[0] + redv[1]) + redv[2]) + redv[3];
      // c and dc columns of this lane in registers for all frames (only the h rows are read per frame)
      float4 cvr[NVA], dvr[NVA];
#pragma unroll
      for (int i = 0; i < NVA; ++i) {
        const int a4 = lane + 64 * i;
        cvr[i] = a4 < A / 4 ? reinterpret_cast<const float4*>(cs_)[a4] : make_float4(0.f, 0.f, 0.f, 0.f);
        dvr[i] = a4 < A / 4 ? reinterpret_cast<const float4*>(dcs)[a4] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      // the wave's frames in groups of four: the four frames' h loads issued together, the four dot products as
      // independent chains, then their four DPP reductions.  Branch-free (as F2's scores): a frame past the wave's
      // share or past the utterance reads a valid row of the chunk and its product is dropped by a select
      const int lmax = min(XLC, L - ch * XLC) - 1;  // last row of the chunk
#pragma unroll
      for (int i0 = 0; i0 < XM / 4; i0 += 4) {  // compile-time bound: alv stays in registers
        if (i0 >= FPW) break;
        float4 hv4[4][NVA];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int li = min(wave * FPW + min(i0 + u, FPW - 1), lmax);
          const float4* hl4 = reinterpret_cast<const float4*>(hres + (long)li * A);
#pragma unroll
          for (int i = 0; i < NVA; ++i) {
            const int a4 = lane + 64 * i;
            hv4[u][i] = a4 < A / 4 ? hl4[a4] : make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
        float dd[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          floatx2 s2 = {0.f, 0.f};  // (.x, .y: the scalar form's s0, s1, bitwise)
#pragma unroll
          for (int i = 0; i < NVA; ++i) {  // (cvr / dvr are 0 on columns past A: the terms drop out)
            const float4 hv = hv4[u][i], cv = cvr[i], dv = dvr[i];
            s2 = pk_fma(floatx2{hv.x, hv.y} - floatx2{cv.x, cv.y}, floatx2{dv.x, dv.y}, s2);
            s2 = pk_fma(floatx2{hv.z, hv.w} - floatx2{cv.z, cv.w}, floatx2{dv.z, dv.w}, s2);
          }
          const int l = ch * XLC + wave * FPW + i0 + u;
          dd[u] = (i0 + u < FPW && l < L) ? s2.x + s2.y : 0.f;
        }
        // the four frames' dots in one transposed reduction: lanes 0-3 hold them (wave_sum4_slot)
        const float tot = wave_sum4_t(dd[0], dd[1], dd[2], dd[3], lane);
        if (lane < 4) {
          const int u = wave_sum4_slot(lane), i = i0 + u, li = wave * (FPW) + i, l = ch * XLC + li;
          const float au = u == 0 ? alv[i0] : u == 1 ? alv[i0 + 1] : u == 2 ? alv[i0 + 2] : alv[i0 + 3];
          if (i < FPW) {
            float de = 0.f;
            if (l < L) {
              de = au * (tot + (lam * (float)(Lu - l) * (ind - indn) - spen));
              x.DE[arow * L + l] = de;
            }
            des[li] = de;
          }
        }
      }
      XSTAMP(8);  // sub-phase: this wave's de done
      __syncthreads();
      XSTAMP(9);  // sub-phase: all de in LDS
      // partial dws[j] = sum_l de_l we_j (g_lj - gref_j), g_lj = 1 - tanh^2(ws_j + Vh_lj), thread per
      // column j.  sum_l de_l = 0 (softmax), so any gref common to all chunks of the utterance leaves
      // the total unchanged; gref_j = g at the utterance's mean Vh row shrinks the terms, and with them
      // the fp32 cancellation of sum_l de_l g_lj (the reference's dws / dbs are such small sums)
      const int lend = min(XLC, L - ch * XLC);
      const long poff = sl * (long)B * NCH * SC + ((long)ub * NCH + ch) * SC;
      // four frames per pass into four partial sums per column (frame i into sum i % 4), the thread's NJ columns in
      // the same pass: 4 NJ independent chains (one column after the other left half of them to the scheduler).
      // g - gref = 4 r (1 - r) - gref (tanh_r); we_j multiplies the chunk's sum once
      int jq[NJ];
      float acc4[NJ][4], ngr[NJ];
#pragma unroll
      for (int q = 0; q < NJ; ++q) {
        jq[q] = min(tid + 256 * q, SC - 1);  // (columns past SC: a valid column, not published)
        ngr[q] = -grf[q];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc4[q][u] = 0.f;
      }
      // product form (pf, uniform): r = 1 / (E W + 1) with W = 2^(K ws_j) once per column
      float wq[NJ];
#pragma unroll
      for (int q = 0; q < NJ; ++q) wq[q] = pf ? __builtin_amdgcn_exp2f(wsj[q]) : 0.f;
      auto dws_terms = [&](auto pfc) {
        constexpr bool PF = decltype(pfc)::value;
        auto r_of = [&](float v, int q) -> float {
          if constexpr (PF) return __builtin_amdgcn_rcpf(fmaf(RES == 0 ? pf_e(v) : v, wq[q], 1.f));
          else return tanh_r(fmaf(v, kTanhK, wsj[q]));
        };
        int i = 0;
        for (; i + 4 <= lend; i += 4) {
          const float4 d4 = *reinterpret_cast<const float4*>(&des[i]);
          const floatx2 dv2[2] = {floatx2{d4.x, d4.y}, floatx2{d4.z, d4.w}};
          float vv[NJ][4];
#pragma unroll
          for (int q = 0; q < NJ; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u) vv[q][u] = vres[(long)(i + u) * SC + jq[q]];
          // frames in packed pairs (the scalar form's four sums per column, bitwise)
          const floatx2 four2 = {4.f, 4.f};
#pragma unroll
          for (int q = 0; q < NJ; ++q) {
            const floatx2 ng2 = {ngr[q], ngr[q]};
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              const floatx2 rr = {r_of(vv[q][2 * p], q), r_of(vv[q][2 * p + 1], q)};
              const floatx2 a = pk_fma(dv2[p], pk_fma(four2, pk_fma(-rr, rr, rr), ng2),
                                       floatx2{acc4[q][2 * p], acc4[q][2 * p + 1]});
              acc4[q][2 * p] = a.x;
              acc4[q][2 * p + 1] = a.y;
            }
          }
        }
        for (int u = 0; i < lend; ++i, ++u) {
#pragma unroll
          for (int q = 0; q < NJ; ++q) {
            const float rr = r_of(vres[(long)i * SC + jq[q]], q);
            acc4[q][u] = fmaf(des[i], fmaf(4.f, fmaf(-rr, rr, rr), ngr[q]), acc4[q][u]);
          }
        }
      };
      if (pf) dws_terms(std::true_type{});
      else dws_terms(std::false_type{});
#pragma unroll
      for (int q = 0; q < NJ; ++q) {
        const int j = tid + 256 * q;
        if (j < SC)
          put_granule(x.gPDWS + poff + j, ejj[q] * ((acc4[q][0] + acc4[q][1]) + (acc4[q][2] + acc4[q][3])), tag, loc);
      }
      if (!b4ok) return;
    }
    XSTAMP(4);
    // ---- B45: dws = sum over the utterance's chunks (fixed order) -> DWS and granules
    if (rdw) {
      const int cb = b0 + w / nsg, j = 256 * (w % nsg) + tid;
      const bool col = j < SC;
      const granule_t* P = x.gPDWS + sl * (long)B * NCH * SC + (long)cb * NCH * SC;
      float v[kXMaxCh];
      bool ok = true;
      if (col) {
        ok = NCH <= 8 ? poll_column<8>(P, NCH, SC, j, tag, v, abort_word)
                      : poll_column<kXMaxCh>(P, NCH, SC, j, tag, v, abort_word);
        float s = 0.f;
        for (int q = 0; q < NCH; ++q) s += v[q];
        if (loc) put_sent(x.sDWS + p * sSc + sidx(SC, cb, j), s);
        else put_granule(x.gDWS + sl * sSc + (long)cb * SC + j, s, tag);
        k.DWS[((long)cb * T + t) * SC + j] = s;
      }
      if (!ok) abort_lds = 1;  // no LDS data crosses waves in B45: agreed on at B5's reduce
    }
    XSTAMP(5);
    // ---- B5: ds_{t-1} = ((dsp + us') + Ws^T dws) + ds_mlp_{t-1}
    if (sw && t > 0) {
      const Act nxt = load_act(t - 1);
      float4 av[NSC];
      const bool ok =
          loc ? sweep_sent<NSC>(av, rsrc_of(x.sDWS), soff(p * sSc, SC), wave, lane, abort_word, km)
              : sweep_skinny<NSC>(av, rsrc_of(x.gDWS), 8 * (sl * sSc + (long)br * SC), tag, wave, lane, abort_word);
      const floatx4 a1 = mfma_rows_aw<R4, NSC>(av, wsT, lane);
      float v;
      const bool b5ok = dec_sync(red, &abort_lds, ok, a1, wave, lane, tid, &v);
      const float carry = (dsp + usp) + v;
      ds = live ? nxt.dv + carry : 0.f;
      cur = nxt;
      if (!b5ok) return;
    }
    XSTAMP(6);
  }
}

// dVh[b,l,j] = we_j sum_t de_{t,l} (1 - tanh^2(ws_tj + Vh_lj)); DWEACC[b*NCH16 + l/16][j] = sum over the
// 16-frame block's frames and all t of de tanh (colsum'd into dwe by attn_bwd_wgrad).
// grid (Sc/64, ceil(L/32), B): 64 columns x 32 frames (two 16-frame blocks) per workgroup; ws_t of the 64 columns and
// de of the 32 frames staged in LDS; thread = (column, group of 8 frames): per t one LDS read of ws and two float4 of
// de feed 8 independent tanh chains (16 frames per workgroup and 4 chains per thread: 27.8 us at config 2).
constexpr int kDvhMaxT = 256, kDvhF = 32;
// dynamic LDS: ws [T][64] | de [T][32]  (dec_xcd_dvh_lds)
__host__ __device__ constexpr size_t dec_xcd_dvh_lds(int T) { return sizeof(float) * (size_t)T * (64 + kDvhF); }
// Product form of the terms (when every |K ws| and |K Vh| of the workgroup is <= 63, so 2^(K ws) 2^(K Vh) stays a
// normal float): r = 1 / (2^(K Vh) 2^(K ws_t) + 1) -- 2^(K Vh) once per thread, 2^(K ws_t) once per t for the
// thread's eight frames -- instead of 1 / (2^(K (ws + Vh)) + 1) per term: one v_exp per eight terms instead of one
// each.  Outside that range the workgroup takes the per-term form (a uniform branch).
__device__ int g_dvh_force_wide = 0;  // s2s_debug_dvh_wide(1) (tests): the per-term form everywhere
__global__ __launch_bounds__(256) void dec_xcd_dvh(AttnK k, XArgs x) {
  constexpr int F = kDvhF, Q = F / 4;  // frames per workgroup, per thread
  extern __shared__ __attribute__((aligned(16))) float dvl[];
  float (*wsl)[64] = reinterpret_cast<float (*)[64]>(dvl);           // [t][column in slice]
  float (*del)[F] = reinterpret_cast<float (*)[F]>(dvl + 64 * k.T);  // [t][frame in block]
  __shared__ float dw[4][64];
  __shared__ int wide_lds;  // some |K ws| or |K Vh| > 63: per-term form
  const int tid = threadIdx.x, cg = blockIdx.x, blk = blockIdx.y, b = blockIdx.z;
  const int L = k.L, T = k.T, SC = k.Sc;
  const int l0 = blk * F, lend = min(F, L - l0);
  const int j0 = cg * 64;
  if (tid == 0) wide_lds = g_dvh_force_wide;
  // the de / ws slices are staged with eight loads per thread in flight (one at a time, the staging was most of the
  // launch at T = 200: its 75 dependent round trips per thread)
  for (int i0 = tid; i0 < T * F; i0 += 8 * 256) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = i0 + q * 256, t = i / F, f = i % F;
      v[q] = (i < T * F && f < lend) ? x.DE[((long)b * T + t) * L + l0 + f] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = i0 + q * 256;
      if (i < T * F) del[i / F][i % F] = v[q];
    }
  }
  const int jl = tid & 63, fg = tid >> 6, j = j0 + jl;
  float vh[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int f = fg * Q + q;
    vh[q] = (j < SC && f < lend) ? k.Vh[((long)b * L + l0 + f) * SC + j] : 0.f;
  }
  __syncthreads();  // wide_lds initialised
  bool wide = false;
  for (int i0 = tid; i0 < T * 64; i0 += 8 * 256) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = i0 + q * 256, t = i / 64, c = i % 64;
      v[q] = (i < T * 64 && j0 + c < SC) ? kTanhK * k.WS[((long)b * T + t) * SC + j0 + c] : 0.f;  // K ws (tanh_r)
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = i0 + q * 256;
      if (i < T * 64) {
        wsl[i / 64][i % 64] = v[q];
        wide |= !(fabsf(v[q]) <= 63.f);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) wide = wide || !(fabsf(kTanhK * vh[q]) <= 63.f);
  if (wide) wide_lds = 1;
  __syncthreads();
  float dwe = 0.f;
  if (j < SC) {
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    if (wide_lds == 0) {
      // The loop is VALU-issue-bound (a wave64 FMA holds its SIMD 4 cycles, v_rcp 8): per term one FMA for the
      // denominator, the v_rcp, two FMAs for de r (1 - r) and two for de (1 - 2 r); the 4 of 4 r (1 - r) is applied
      // once at the end (28.7 -> 23.2 us per launch at config 2).  Frames in pairs (packed fp32 FMAs).  (dwe as
      // -2 sum de r -- sum_l de_l = 0 in exact arithmetic -- missed 1e-4 on long utterances: the rounding of the de
      // values does not cancel.)
      typedef float f2 __attribute__((ext_vector_type(2)));
      f2 ev[Q / 2], a2[Q / 2], w2[Q / 2];
#pragma unroll
      for (int q = 0; q < Q / 2; ++q) {
        ev[q] = f2{__builtin_amdgcn_exp2f(kTanhK * vh[2 * q]), __builtin_amdgcn_exp2f(kTanhK * vh[2 * q + 1])};
        a2[q] = f2{0.f, 0.f};
        w2[q] = f2{0.f, 0.f};
      }
      const f2 one = {1.f, 1.f}, m2 = {-2.f, -2.f};
      for (int t = 0; t < T; ++t) {
        const float e1 = __builtin_amdgcn_exp2f(wsl[t][jl]);
        const f2 ew = {e1, e1};
        const float4 da = *reinterpret_cast<const float4*>(&del[t][fg * Q]);
        const float4 db = *reinterpret_cast<const float4*>(&del[t][fg * Q + 4]);
        const f2 d2[Q / 2] = {f2{da.x, da.y}, f2{da.z, da.w}, f2{db.x, db.y}, f2{db.z, db.w}};
#pragma unroll
        for (int q = 0; q < Q / 2; ++q) {  // tanh = 1 - 2 r, 1 - tanh^2 = 4 r (1 - r)
          const f2 den = __builtin_elementwise_fma(ev[q], ew, one);
          const f2 r = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
          a2[q] = __builtin_elementwise_fma(d2[q], __builtin_elementwise_fma(-r, r, r), a2[q]);
          w2[q] = __builtin_elementwise_fma(d2[q], __builtin_elementwise_fma(m2, r, one), w2[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < Q / 2; ++q) {
        acc[2 * q] = 4.f * a2[q].x;
        acc[2 * q + 1] = 4.f * a2[q].y;
      }
      dwe = ((w2[0].x + w2[0].y) + (w2[1].x + w2[1].y)) + ((w2[2].x + w2[2].y) + (w2[3].x + w2[3].y));
    } else {
      for (int t = 0; t < T; ++t) {
        const float w = wsl[t][jl];
        const float4 da = *reinterpret_cast<const float4*>(&del[t][fg * Q]);
        const float4 db = *reinterpret_cast<const float4*>(&del[t][fg * Q + 4]);
        const float d8[Q] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const float r = tanh_r(fmaf(vh[q], kTanhK, w));
          acc[q] = fmaf(d8[q], 4.f * fmaf(-r, r, r), acc[q]);
          dwe = fmaf(d8[q], fmaf(-2.f, r, 1.f), dwe);
        }
      }
    }
    const float ej = k.P.we[j];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int f = fg * Q + q;
      if (f < lend) k.DVH[((long)b * L + l0 + f) * SC + j] = ej * acc[q];
    }
  }
  dw[fg][jl] = dwe;
  __syncthreads();
  // the two 16-frame blocks' sums (frame groups 0-1 and 2-3)
  if (fg < 2 && j < SC && 2 * blk + fg < k.NCH)
    k.DWEACC[((long)b * k.NCH + 2 * blk + fg) * SC + j] = dw[2 * fg][jl] + dw[2 * fg + 1][jl];
}

// VBAR[b][j] = mean over the utterance's own frames of Vh[b, :, j]  (reference point of the dws sums; any point is
// exact, but one that took in the padding frames of a variable-length batch would let their contents into the
// sums' rounding).
// grid (Sc/64, B): 64 columns per workgroup, the frames split over the 4 waves
__device__ __forceinline__ void vbar_body(const AttnK& k, const XArgs& x, int cg, int b) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = cg * 64 + lane;
  const int L = frames_of(k, b), SC = k.Sc;  // (k.L without frame lengths: the same sums as ever)
  float s = 0.f;
  if (j < SC) {
    // eight frames' loads in flight per pass (the sum keeps its frame order): a 64-block launch, so each thread's
    // chain of L / 4 loads is the launch's length (the merged head launch 20.4 -> 17.9 us at config 2; sixteen
    // in flight: 18.8)
    const float* v = k.Vh + ((long)b * k.L) * SC + j;
    int l = wave;
    for (; l + 28 < L; l += 32) {
      float q[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = v[(long)(l + 4 * i) * SC];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += q[i];
    }
    for (; l < L; l += 4) s += v[(long)l * SC];
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && j < SC)
    x.VBAR[(long)b * SC + j] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) * (1.0f / (float)L);
}
__global__ __launch_bounds__(256) void dec_xcd_vbar(AttnK k, XArgs x) { vbar_body(k, x, blockIdx.x, blockIdx.y); }
// after the XCD-local forward, one launch: alpha / MonotonicAlignment indicators (blocks [0, T B)) and VBAR
// (the next ceil(Sc / 64) B blocks) -- both only read by the backward (and alpha()), so VBAR is no longer a
// launch between the Vh GEMM and the decoder
__global__ __launch_bounds__(256) void dec_xcd_alpha_vbar(AttnK k, XArgs x) {
  const int nab = k.T * k.B, bid = blockIdx.x;
  if (bid < nab) {
    alpha_ind_body(k, bid % k.T, bid / k.T);
  } else {
    const int v = bid - nab, ncg = (k.Sc + 63) / 64;
    vbar_body(k, x, v % ncg, v / ncg);
  }
}
// the same two jobs and, in the blocks after them, the MLP head over all B T rows (mlp_head_body): the model
// step's launch after the decoder's MLP GEMM (alpha / VBAR are not a launch of their own between the
// decoder and that GEMM)
__global__ __launch_bounds__(256) void dec_xcd_alpha_vbar_head(AttnK k, XArgs x, int rows) {
  const int nab = k.T * k.B, ncg = (k.Sc + 63) / 64, nvb = ncg * k.B, bid = blockIdx.x;
  if (bid < nab) {
    alpha_ind_body(k, bid % k.T, bid / k.T);
  } else if (bid < nab + nvb) {
    const int v = bid - nab;
    vbar_body(k, x, v % ncg, v / ncg);
  } else {
    mlp_head_body(k, rows, bid - nab - nvb);
  }
}

// y_in_t = Wy[:, y_{t-1}] + by (by at t = 0) into CY[:, S:]   (Attention.lua:149, RNNAttention.lua:172-176)
__global__ void dec_xcd_yin(AttnK k) {
  const int S = k.S;
  const long n = (long)k.B * k.T * S;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / S;
    const int j = (int)(i - row * S);
    const int t = (int)(row % k.T);
    float v = k.P.by[j];
    if (t > 0) v += k.P.Wy[(long)j * k.O + k.labels[row - 1]];
    k.CY[row * 2 * S + S + j] = v;
  }
}

// The prologue's parameter re-layouts and y_in in ONE launch (its kernels only run in the gaps between
// the persistent GRU launches, so fewer launches = a shorter tail after the encoder):
//   WXD  = [Wz_d; Wr_d; Wh_d] (the d-columns of the decoder GRU, 3S x S)
//   XWHT = Wh[:, :S]^T, XZRT = [Wz[:, :S]; Wr[:, :S]]^T, XWST = Ws^T (backward operand layouts)
//   CY[:, S:] = y_in = Wy[:, y_{t-1}] + by (t > 0), by (t = 0)
__global__ void dec_xcd_pack_ops(AttnK k, XArgs x) {
  const int S = k.S, Sc = k.Sc, A = k.A;
  // s_0 = 0 (Recurrent.lua:112 zeros_hidden; dec_init_fwd's work, done here off the decoder's critical path)
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (long)k.B * S; i += (long)gridDim.x * blockDim.x) {
    const long b = i / S, n = i - b * S;
    k.HX[(b * k.T) * 2 * S + n] = 0.f;
  }
  const long SS = (long)S * S, n0 = 3 * SS, n1 = n0 + SS, n2 = n1 + 2 * SS, n3 = n2 + (long)S * Sc,
             n4 = n3 + (long)k.B * k.T * S;
  // the prologue GEMMs' transposed operands: PWDYT = Wd[:, S:]^T, PWDCT = Wd[:, :S]^T, PWCT = Wc^T,
  // PWXDT = WXD^T (S x 3S, read from the Wz / Wr / Wh d-columns directly)
  const long m0 = n4 + SS, m1 = m0 + SS, m2 = m1 + (long)A * S, m3 = m2 + 3 * SS;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < m3; i += (long)gridDim.x * blockDim.x) {
    if (i >= n4) {
      if (i < m0) {
        const long e = i - n4;
        const int c = (int)(e / S), n = (int)(e - (long)c * S);
        x.PWDYT[e] = k.P.Wd[(long)n * 2 * S + S + c];
      } else if (i < m1) {
        const long e = i - m0;
        const int c = (int)(e / S), n = (int)(e - (long)c * S);
        x.PWDCT[e] = k.P.Wd[(long)n * 2 * S + c];
      } else if (i < m2) {
        const long e = i - m1;
        const int a = (int)(e / S), n = (int)(e - (long)a * S);
        x.PWCT[e] = k.P.Wc[(long)n * A + a];
      } else {
        const long e = i - m2;
        const int c = (int)(e / (3 * S)), j = (int)(e - (long)c * 3 * S), g = j / S, n = j - g * S;
        const float* W = g == 0 ? k.P.Wz : g == 1 ? k.P.Wr : k.P.Wh;
        x.PWXDT[e] = W[(long)n * 2 * S + S + c];
      }
      continue;
    }
    if (i < n0) {
      const int g = (int)(i / SS);
      const long rem = i - g * SS;
      const int n = (int)(rem / S), c = (int)(rem - (long)n * S);
      const float* W = g == 0 ? k.P.Wz : g == 1 ? k.P.Wr : k.P.Wh;
      x.WXD[i] = W[(long)n * 2 * S + S + c];
    } else if (i < n1) {
      const long e = i - n0;
      const int c = (int)(e / S), n = (int)(e - (long)c * S);
      x.XWHT[e] = k.P.Wh[(long)n * 2 * S + c];
    } else if (i < n2) {
      const long e = i - n1;
      const int c = (int)(e / (2 * S)), j = (int)(e - (long)c * 2 * S);
      x.XZRT[e] = j < S ? k.P.Wz[(long)j * 2 * S + c] : k.P.Wr[(long)(j - S) * 2 * S + c];
    } else if (i < n3) {
      const long e = i - n2;
      const int c = (int)(e / Sc), r = (int)(e - (long)c * Sc);
      x.XWST[e] = k.P.Ws[(long)r * S + c];
    } else {
      const long e = i - n3;
      const long row = e / S;
      const int j = (int)(e - row * S);
      const int t = (int)(row % k.T);
      float v = k.P.by[j];
      if (t > 0) v += k.P.Wy[(long)j * k.O + k.labels[row - 1]];
      k.CY[row * 2 * S + S + j] = v;
    }
  }
}

// bkd = Wd[:, :S] bc + bd   (one wave per output)
__global__ void dec_xcd_bkd(AttnK k, float* bkd) {
  const int S = k.S, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= S) return;
  float s = 0.f;
  for (int c = lane; c < S; c += 64) s += k.P.Wd[(long)n * 2 * S + c] * k.P.bc[c];
  s = wave_sum(s);
  if (lane == 0) bkd[n] = s + k.P.bd[n];
}
