// Attention decoder forward/backward: the drop-in for nn.Attention's decoder graph
// (Attention.lua:43-211, 305-327) unrolled by nn.RNNAttention (RNNAttention.lua:144-253)
// with the Chorowski decoder_recurrent / decoder_mlp (timit/model_chorowski_baseline.lua:48-59).
//
// Per decoder step t (teacher forcing, RNNAttention.lua:172-176), one launch each:
//   F1 ws = Ws s_{t-1} + bs                           skinny MFMA  (Attention.lua:65-66)
//   F2 e_l = we . tanh(ws + Vh_l); local softmax stats
//      and partial context over a 16-frame chunk       wave-dot + wave reductions (Attention.lua:98-117, 132-134)
//   F3 combine chunks -> alpha, c, lse, MonoAlign ind  (MonotonicAlignment.lua:19-42)
//   F4 c_in = Wc c + bc, y_in = Wy[:,y_{t-1}] + by      skinny MFMA  (Attention.lua:149-150)
//   F5 d = Wd [c_in; y_in] + bd                        skinny MFMA  (Attention.lua:151)
//   F6/F7 decoder GRU (GRU.lua:22-30) on [s_{t-1}; d]   skinny MFMA x2
// The decoder MLP (Maxout -> Linear -> LogSoftMax) is not on the recurrence, so it runs
// once for all B*T rows after the loop (one GEMM + one per-row head kernel).
// Backward mirrors RNNAttention:updateGradInput's reverse loop (RNNAttention.lua:233-250):
// MLP backward for all rows first, then per step GRU p1/p2, Wd^T, Wc^T, the fused
// attention backward (softmax, tanh, dVh, dh += alpha dc), the dws combine and Ws^T;
// every weight gradient is one GEMM over all B*T rows afterwards.
#include "attn.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "decisions.h"
#include "attn_k.h"
#include "skinny.h"

namespace s2s {
#include "attn_layout.inc"
namespace {
#include "dec_steps.inc"
#include "attn_persist.inc"
#include "dec_xcd.inc"
#include "dec_xcd_lstm.inc"
}  // namespace

int attn_check_dims(const AttnDims& d) {
  S2S_REQUIRE(d.B > 0 && d.L > 0 && d.T > 0, "attn: empty B/L/T");
  S2S_REQUIRE(d.S % 16 == 0 && d.A % 16 == 0 && d.Sc % 16 == 0, "attn: S, A, scoreDepth must be multiples of 16");
  S2S_REQUIRE(d.Sc <= 1024, "attn: scoreDepth > 1024 not supported");
  S2S_REQUIRE(d.O > 0 && d.M > 0 && d.K > 0, "attn: bad output/mlp dims");
  S2S_REQUIRE(!d.ext || d.dropout == 0.f, "attn: dropout belongs to the external decoder_mlp");
  S2S_REQUIRE(d.dropout >= 0.f && d.dropout < 1.f, "attn: dropout must be in [0, 1)");
  S2S_REQUIRE(d.hf >= 0 && (d.hf == 0 || (d.hk >= 1 && d.hk <= kMaxHybK)),
              "attn: hybridAttendFilterSize must be in [1, 8] when hybridAttendFeatureMaps > 0");
  return 0;
}
static std::atomic<unsigned long long*> g_dec_stamps[2] = {{nullptr}, {nullptr}};

// algorithmic flops of one decoder recurrence launch (T P_step + T L (2 Sc + A) per utterance,
// times 2; the backward does twice the forward's products)
static double dec_flops(const AttnDims& d, bool bwd) {
  const double S = d.S, Sc = d.Sc, A = d.A, O = d.O, Mk = (double)d.M * d.K;
  const double p_step = S * Sc + O * S + A * S + 2 * S * S + 3 * S * 2 * S + (S + A) * Mk + d.M * O;
  const double f = 2.0 * d.B * ((double)d.T * p_step + (double)d.T * d.L * (2 * Sc + A));
  return bwd ? 2.0 * f : f;
}

// A persistent launch must be fully co-resident (its workgroups wait on each other).
static bool co_resident(const void* fn, int grid, size_t dyn_lds) {
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
  if (dyn_lds > 0 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds) != hipSuccess)
    return false;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, dyn_lds) != hipSuccess) return false;
  return (long)per_cu * cus >= grid;
}

// resident-chunk variant (attn_persist.inc) when the chunks fit
static bool dec_res_enabled(const AttnDims& d) { return 16 * ((d.L + LC - 1) / LC) <= kDecWG; }

struct PersistLaunch {
  const void* fn = nullptr;
  size_t lds = 0;
  int res = -1;  // 1: the resident-chunk candidate, 0: the other one (the decision record's dec.persist_res)
};
// The persistent kernel to launch for width variant `var`: the resident-chunk candidate where the chunks fit, else the
// streaming one, each only if co-resident.  fn = nullptr: neither is (the caller issues the per-step launches).
static PersistLaunch pick_dec(bool fwd, int var, const AttnDims& d, int grid) {
  const void* const fns[2][2][2] = {  // [fwd, bwd][variant 1, 2][resident, streaming]
      {{(const void*)dec_fwd_persist<4, 8, 2, true>, (const void*)dec_fwd_persist<4, 8, 2, false>},
       {(const void*)dec_fwd_persist<1, 2, 1, true>, (const void*)dec_fwd_persist<1, 2, 1, false>}},
      {{(const void*)dec_bwd_persist<4, 8, true>, (const void*)dec_bwd_persist<4, 8, false>},
       {(const void*)dec_bwd_persist<1, 2, true>, (const void*)dec_bwd_persist<1, 2, false>}}};
  const void* const* f = fns[fwd ? 0 : 1][var == 1 ? 0 : 1];
  const PersistLaunch c[2] = {{f[0], fwd ? dec_fwd_res_lds(d.A, d.Sc) : dec_bwd_res_lds(d.A, d.Sc), 1}, {f[1], 0, 0}};
  for (int i = dec_res_enabled(d) ? 0 : 1; i < 2; ++i)
    if (co_resident(c[i].fn, grid, c[i].lds)) return c[i];
  return {};
}
static int launch_persist(const PersistLaunch& p, int grid, hipStream_t st, AttnK& k) {
  void* args[] = {&k};
  S2S_TRY(check_resident(p.fn, grid, 256, p.lds, "decoder persistent launch"));
  S2S_CHECK_HIP(hipLaunchKernel(p.fn, dim3(grid), dim3(256), args, p.lds, st));
  return 0;
}

// The decision record (decisions.h) of one decoder launch, by the path function that issues it: the path that ran, the
// XCD-local plan as handed to the kernel (0 on the other paths), the pick_dec candidate that was launched (-1: none).
static void record_dec_launch(bool fwd, int path, const XPlan& xp, const XArgs& x, int persist_res) {
  decide(fwd ? "dec.fwd.path" : "dec.bwd.path", path);
  const bool xcd = path >= 2;
  decide("dec.var", xcd ? xp.var : 0);
  decide("dec.U", xcd ? x.U : 0);
  decide("dec.nchains", xcd ? x.nchains : 0);
  decide("dec.XLC", xcd ? x.XLC : 0);
  decide("dec.NCH", xcd ? x.NCH : 0);
  decide("dec.res", xcd ? xp.res : -1);
  decide("dec.allow_local", xcd ? x.allow_local : 0);
  decide("dec.persist_res", persist_res);
}

static std::atomic<int> g_dec_allow_local{1};
// s2s_debug_head_sums_slabs(0) (A/B): the decoder MLP GEMM's split-K reduce as its own launch in front of the MLP head
static std::atomic<int> g_head_sums_slabs{1};
static std::atomic<int> g_merge_alpha_head{1};  // s2s_debug_merge_alpha_head(0) (diagnostic): alpha / VBAR launched alone
// attn_fwd's merged launch after the MLP GEMM: alpha / indicators, VBAR and the MLP head (the XCD-local paths, no split
// side stream, the in-library MLP)
static bool merged_head(const AttnDims& d, const DecRoute& r, hipStream_t side) {
  return r.xcd() && !side && !d.ext && g_merge_alpha_head;
}
// ... which also runs the head's backward when the seed is final before the forward (AttnDims::dlogp_early); bwd_mlp
// then launches none.  attn_fwd refuses dlogp_early with a side stream, so both sides decide alike without one.
static bool attn_head_bwd_fused(const AttnDims& d, const DecRoute& r) {
  return d.dlogp_early && merged_head(d, r, nullptr);
}

// s2s_debug_dec_r4(0) (A/B): chains of <= 4 utterances keep the 16 x 16 x 4 skinny products
static std::atomic<int> g_dec_r4{1};
static std::atomic<int> g_dec_pf_host{1};  // what s2s_debug_dec_pf last wrote to the device's g_dec_pf (decision record)
template <int S, int A, int SC, bool R4>
static const void* xcd_kernel(bool fwd, int res) {
  return res == 2 ? (fwd ? (const void*)dec_xcd_fwd<S, A, SC, 2, R4> : (const void*)dec_xcd_bwd<S, A, SC, 2, R4>)
       : res == 1 ? (fwd ? (const void*)dec_xcd_fwd<S, A, SC, 1, R4> : (const void*)dec_xcd_bwd<S, A, SC, 1, R4>)
                  : (fwd ? (const void*)dec_xcd_fwd<S, A, SC, 0, R4> : (const void*)dec_xcd_bwd<S, A, SC, 0, R4>);
}
template <int S, int A, int SC>
static int launch_xcd_t(bool fwd, int res, hipStream_t st, AttnK& k, XArgs& x) {
  const size_t lds = xdec_lds<S, A, SC>(x.XLC, res);
  // a chain of at most 4 utterances (B <= 32): its skinny products on the 4 x 4 x 1 MFMA (handoff.h mfma4_aw_acc)
  const bool r4 = x.U <= 4 && g_dec_r4.load();
  const void* fn = r4 ? xcd_kernel<S, A, SC, true>(fwd, res) : xcd_kernel<S, A, SC, false>(fwd, res);
  decide("dec.r4", r4);
  decide("dec.pf", g_dec_pf_host.load());
  if (lds) S2S_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  void* args[] = {&k, &x};
  S2S_TRY(check_resident(fn, chain_grid(x.nchains, kXWG), 256, lds, fwd ? "dec_xcd_fwd" : "dec_xcd_bwd"));
  S2S_CHECK_HIP(hipLaunchKernel(fn, dim3(chain_grid(x.nchains, kXWG)), dim3(256), args, lds, st));
  return 0;
}
static int launch_xcd(const XPlan& xp, bool fwd, hipStream_t st, AttnK& k, XArgs& x) {
  if (xp.var == 1) return launch_xcd_t<256, 512, 512>(fwd, xp.res, st, k, x);
  return launch_xcd_t<64, 128, 128>(fwd, xp.res, st, k, x);
}
// the LSTM / hybrid kernels (var 3: S = 400 carried as 448, A = 256, Sc = 160, resident chunks, 4 x 4 x 1 products)
static int launch_xcd_lstm(bool fwd, hipStream_t st, AttnK& k, XArgs& x, XLArgs& y) {
  const size_t lds = xdec_lds<kXlSP, 256, 160>(x.XLC, 2);
  const void* fn = fwd ? (const void*)dec_xcd_lstm_fwd<kXlSP, 256, 160, 5, true>
                       : (const void*)dec_xcd_lstm_bwd<kXlSP, 256, 160, kXlSCP, 5, true>;
  if (lds) S2S_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  void* args[] = {&k, &x, &y};
  decide("dec.r4", 1);
  S2S_TRY(check_resident(fn, chain_grid(x.nchains, kXWG), 256, lds, fwd ? "dec_xcd_lstm_fwd" : "dec_xcd_lstm_bwd"));
  S2S_CHECK_HIP(hipLaunchKernel(fn, dim3(chain_grid(x.nchains, kXWG)), dim3(256), args, lds, st));
  return 0;
}

// Folds and teacher-forced constants of the LSTM / hybrid kernels (params and labels only): the re-layouts, y_in,
// BKD, the hybrid fold (HGT, HCU), WDC = Wd_c Wc, KD = y_in Wd_y^T + BKD, then per gate q: WXG_q = Wq_x WDC and
// KXG_q = KD Wq_x^T + bq (the padded rows / columns stay zero), WXGT = WXG^T.
static int dec_xcd_lstm_prologue(hipStream_t st, const AttnDims& d, AttnK& k, const XArgs& x, const XLArgs& y,
                                 const GemmWs& gws) {
  WgradPrecision wp;  // the folds are reused by every step: fp32
  const int S = d.S, A = d.A, rows = d.B * d.T;
  const long SP = kXlSP;
  hipLaunchKernelGGL(dec_xcd_lstm_pack, dim3(1024), dim3(256), 0, st, k, y, kXlSP, kXlSCP);
  hipLaunchKernelGGL(dec_xcd_bkd, dim3((S + 3) / 4), dim3(256), 0, st, k, x.BKD);
  hipLaunchKernelGGL(dec_hyb_fold, dim3((d.Sc + 255) / 256), dim3(256), 0, st, k);
  S2S_CHECK_HIP(hipGetLastError());
  S2S_TRY(zero_async(st, y.WXG, sizeof(float) * 4 * SP * A));
  S2S_TRY(zero_async(st, y.KXG, sizeof(float) * (size_t)rows * 4 * SP));
  S2S_TRY(gemm1(st, false, false, S, A, S, 1.f, k.P.Wd, 2L * S, k.P.Wc, A, 0.f, x.WDC, A, nullptr, gws));
  S2S_TRY(gemm1(st, false, true, rows, S, S, 1.f, k.CY + S, 2L * S, k.P.Wd + S, 2L * S, 0.f, x.KD, S, x.BKD, gws));
  GemmProblem pw[4], pk[4];
  for (int q = 0; q < 4; ++q) {
    pw[q] = GemmProblem{y.WXD4 + (long)q * S * S, x.WDC, y.WXG + q * SP * A, nullptr, S, A, A, S, A, S, 1.f, 0.f};
    pk[q] = GemmProblem{x.KD, y.WXD4 + (long)q * S * S, y.KXG + q * SP, y.BQ + (long)q * S, S, S, 4 * SP, rows, S, S,
                        1.f, 0.f};
  }
  S2S_TRY(gemm_f32(st, pw, 4, false, false, gws));
  S2S_TRY(gemm_f32(st, pk, 4, false, true, gws));
  return transpose_f32(st, y.WXG, A, (int)(4 * SP), A, y.WXGT, 4 * SP);
}

// Weight folds and teacher-forced constants of the XCD-local decoder (params and labels only, so
// the model step runs it on the side stream beside the encoder).
static int dec_xcd_prologue(hipStream_t st, const AttnDims& d, AttnK& k, const XArgs& x, const GemmWs& gws) {
  WgradPrecision wp;  // the weight folds Wx' = W_d Wd_c Wc are reused by every step: fp32
  const int S = d.S, A = d.A, rows = d.B * d.T;
  // On the side stream beside the encoder its kernels run only where the persistent GRU launches leave
  // room -- and a kernel with a workgroup dealt to an XCD the layer's chains fill waits for the layer to
  // end -- so the chain is kept to 4 launches: the re-layouts (incl. the transposed operands below) and
  // y_in, BKD, then two batched NN GEMM launches (done by the end of encoder layer 2; the transposes and
  // the separate NT launches of the earlier chain left its last GEMM after layer 3, in front of the decoder)
  hipLaunchKernelGGL(dec_xcd_pack_ops, dim3(1024), dim3(256), 0, st, k, x);
  hipLaunchKernelGGL(dec_xcd_bkd, dim3((S + 3) / 4), dim3(256), 0, st, k, x.BKD);  // BKD = Wd_c bc + bd
  S2S_CHECK_HIP(hipGetLastError());
  // WDC = Wd_c Wc (S x A), WDCT = WDC^T = Wc^T Wd_c^T (A x S), KD = y_in Wd_y^T + BKD (B*T x S)
  const GemmProblem pa[3] = {
      GemmProblem{k.P.Wd, k.P.Wc, x.WDC, nullptr, 2L * S, A, A, S, A, S, 1.f, 0.f},
      GemmProblem{x.PWCT, x.PWDCT, x.WDCT, nullptr, S, S, S, A, S, S, 1.f, 0.f},
      GemmProblem{k.CY + S, x.PWDYT, x.KD, x.BKD, 2L * S, S, S, rows, S, S, 1.f, 0.f}};
  S2S_TRY(gemm_f32(st, pa, 3, false, false, gws));
  // WX = WXD WDC (3S x A), WXT = WX^T = WDC^T WXD^T (A x 3S), KX = KD WXD^T (B*T x 3S)
  const GemmProblem pb[3] = {
      GemmProblem{x.WXD, x.WDC, x.WX, nullptr, S, A, A, 3 * S, A, S, 1.f, 0.f},
      GemmProblem{x.WDCT, x.PWXDT, x.WXT, nullptr, S, 3L * S, 3L * S, A, 3 * S, S, 1.f, 0.f},
      GemmProblem{x.KD, x.PWXDT, x.KX, nullptr, S, 3L * S, 3L * S, rows, 3 * S, S, 1.f, 0.f}};
  S2S_TRY(gemm_f32(st, pb, 3, false, false, gws));
  return 0;
}

// One forward step (k.t) of the per-step path for R rows: F1, F2, F3, F4 + F5 (or their fold, with the WDC / KD of
// the caller's pre-loop GEMMs), then the LSTM or the GRU cell.  f2() launches the attention chunks: dec_f2_attn in
// training, the beam search's own choice in beam.inc.
template <class F2>
static void launch_fwd_step(hipStream_t st, AttnK& k, int R, bool fold, bool lstm, const float* wdc, const float* kd,
                            F2&& f2) {
  const int S = k.S, bt = (R + 15) / 16;
  hipLaunchKernelGGL(dec_f1_ws, dim3(k.Sc / 16, bt), dim3(256), 0, st, k);
  f2();
  hipLaunchKernelGGL(dec_f3_combine, dim3(R), dim3(256), 0, st, k);
  if (fold) {
    hipLaunchKernelGGL(dec_f45_fold, dim3(S / 16, bt), dim3(512), 0, st, k, wdc, kd);
  } else {
    hipLaunchKernelGGL(dec_f4_cin, dim3(S / 16, bt), dim3(256), 0, st, k);
    hipLaunchKernelGGL(dec_f5_d, dim3(S / 16, bt), dim3(256), 0, st, k);
  }
  if (lstm) {
    hipLaunchKernelGGL(dec_f6_lstm, dim3(4 * S / 16, bt), dim3(512), 0, st, k);
  } else {
    hipLaunchKernelGGL(dec_f6_gru1, dim3(2 * S / 16, bt), dim3(256), 0, st, k);
    hipLaunchKernelGGL(dec_f7_gru2, dim3(S / 16, bt), dim3(256), 0, st, k);
  }
}

// One decoder call: the route, resolved here once, the operands carved for it, and one function per path and
// direction.  Each path function says what it expects to be prepared and who writes dh.
struct DecCall {
  hipStream_t st, side;  // side, ev: the caller's split stream and its events (attn.h), or null
  hipEvent_t* ev;
  const AttnDims& d;
  const DecRoute r;
  const GemmWs gws;
  AttnK k{};  // the carved operands
  XArgs x{};
  XLArgs y{};
  bool dh_has_dc = false;  // the backward launch added sum_t alpha_t^T dc_t to dh itself (bwd_persist)
  DecCall(hipStream_t st, const AttnDims& d, const void* saved, void* scratch, hipStream_t side = nullptr,
          hipEvent_t* ev = nullptr)
      : st(st), side(side), ev(ev), d(d), r(dec_route(d)), gws(attn_gemm_ws(d, scratch)) {
    carve(d, &k, (char*)saved, (char*)scratch, &x, &y);
  }
  bool lstm_xcd() const { return r.path == kPathXcdLstm; }
  int prologue() {
    return lstm_xcd() ? dec_xcd_lstm_prologue(st, d, k, x, y, gws) : dec_xcd_prologue(st, d, k, x, gws);
  }
  void set_plan() {  // the plan as the XCD-local kernels read it
    x.U = r.xp.U; x.nchains = r.xp.nchains; x.XLC = r.xp.XLC; x.NCH = r.xp.NCH; x.allow_local = g_dec_allow_local;
  }
  int launch_chains(bool fwd) {
    return lstm_xcd() ? launch_xcd_lstm(fwd, st, k, x, y) : launch_xcd(r.xp, fwd, st, k, x);
  }
  // ---- forward, per-step launches.  Expects Vh.  Writes s_0 and its folds, then T steps; folded, also the c_in rows
  // the weight gradients read.  persist_fallback: the route said persist but no candidate is co-resident (more than two
  // row tiles at one workgroup per CU); attn_sync_regions still names the headers, so they must not be stale memory.
  int fwd_steps(bool persist_fallback) {
    const int B = d.B, S = d.S, A = d.A, rows = B * d.T;
    hipLaunchKernelGGL(dec_init_fwd, dim3((B * S + 255) / 256), dim3(256), 0, st, k);
    ProfScope ps(st, "dec_fwd_steps", 0.0, 0.0);
    record_dec_launch(true, kPathSteps, r.xp, x, -1);
    if (persist_fallback) S2S_TRY(launch_sync_prep(st, k.fsync, 256, nullptr, k.fhdr));
    if (d.hf > 0) hipLaunchKernelGGL(dec_hyb_fold, dim3((d.Sc + 255) / 256), dim3(256), 0, st, k);
    if (d.lstm) hipLaunchKernelGGL(dec_lstm_pack, dim3(256), dim3(256), 0, st, k);
    if (r.fold) {  // y_in rows, BKD = Wd_c bc + bd, WDC = Wd_c Wc, KD = y_in Wd_y^T + BKD
      WgradPrecision wp;  // the folds are reused by every step: fp32
      hipLaunchKernelGGL(dec_fold_yin, dim3(512), dim3(256), 0, st, k);
      hipLaunchKernelGGL(dec_xcd_bkd, dim3((S + 3) / 4), dim3(256), 0, st, k, x.BKD);
      S2S_CHECK_HIP(hipGetLastError());
      S2S_TRY(gemm1(st, false, false, S, A, S, 1.f, k.P.Wd, 2L * S, k.P.Wc, A, 0.f, x.WDC, A, nullptr, gws));
      S2S_TRY(gemm1(st, false, true, rows, S, S, 1.f, k.CY + S, 2L * S, k.P.Wd + S, 2L * S, 0.f, x.KD, S, x.BKD, gws));
    }
    for (int t = 0; t < d.T; ++t) {
      k.t = t;
      launch_fwd_step(st, k, B, r.fold, d.lstm, x.WDC, x.KD,
                      [&] { hipLaunchKernelGGL(dec_f2_attn<8>, dim3(k.NCH, B), dim3(512), 0, st, k); });
    }
    S2S_CHECK_HIP(hipGetLastError());
    // c_in rows for the weight gradients (the folded steps never formed them): CY[:, :S] = C Wc^T + bc
    if (r.fold) S2S_TRY(gemm1(st, false, true, rows, S, A, 1.f, k.C, A, k.P.Wc, A, 0.f, k.CY, 2L * S, k.P.bc, gws));
    return 0;
  }
  // ---- forward, the 7-seam persistent kernel (attn_persist.inc).  Expects Vh.  Writes s_0, zeroes the forward sync
  // region, one launch for all T steps, then alpha / the MonotonicAlignment indicators from the saved scores.
  int fwd_persist() {
    const int pgrid = kDecWG * ((d.B + 15) / 16);
    const PersistLaunch pf = pick_dec(true, r.pvar, d, pgrid);
    if (!pf.fn) return fwd_steps(true);  // the route says persist, the launch has no candidate
    hipLaunchKernelGGL(dec_init_fwd, dim3((d.B * d.S + 255) / 256), dim3(256), 0, st, k);
    S2S_TRY(launch_sync_prep(st, k.fsync, k.fsync_bytes, nullptr, k.fhdr));
    {
      ProfScope ps(st, "dec_fwd_persist", 0.0, 0.0);
      record_dec_launch(true, kPathPersist, r.xp, x, pf.res);
      S2S_TRY(launch_persist(pf, pgrid, st, k));
    }
    hipLaunchKernelGGL(dec_alpha_ind, dim3(d.T, d.B), dim3(256), 0, st, k);
    S2S_CHECK_HIP(hipGetLastError());
    return 0;
  }
  // ---- forward, the XCD-local kernels (dec_xcd.inc, dec_xcd_lstm.inc).  Expects Vh and, if prologue_done,
  // attn_fwd_prologue's folds (they write s_0; with syncs_in_prologue also the zeroed sync regions).  One launch for
  // all T steps; unless the head launch does it (merge_head), alpha / indicators / VBAR (side stream if split: ev[2]).
  int fwd_xcd(bool prologue_done, bool merge_head) {
    if (!prologue_done) S2S_TRY(prologue());
    set_plan();
    const bool synced = d.syncs_in_prologue && prologue_done;
    if (!synced) S2S_TRY(launch_sync_prep(st, k.fsync, k.fsync_bytes, nullptr, k.fhdr));
    {
      // algorithmic units: the attention re-streams Vh and h every step, T B L (Sc + A) 4 bytes
      // per forward; flops = the step products + the attention contractions
      ProfScope ps(st, lstm_xcd() ? "dec_fwd_xcd_lstm" : "dec_fwd_xcd", dec_flops(d, false),
                   4.0 * d.T * d.B * d.L * (double)(d.Sc + d.A));
      record_dec_launch(true, r.path, r.xp, x, -1);
      S2S_TRY(launch_chains(true));
    }
    if (side) {
      S2S_CHECK_HIP(hipEventRecord(ev[1], st));
      S2S_CHECK_HIP(hipStreamWaitEvent(side, ev[1], 0));
    }
    if (!merge_head) {
      hipLaunchKernelGGL(dec_xcd_alpha_vbar, dim3(d.T * d.B + ((d.Sc + 63) / 64) * d.B), dim3(256), 0,
                         side ? side : st, k, x);
      if (side) S2S_CHECK_HIP(hipEventRecord(ev[2], side));
      S2S_CHECK_HIP(hipGetLastError());
    }
    return 0;
  }
  // ---- the decoder MLP over all B*T rows: dropout, U = [s; c] Wm^T + bm, then maxout / Linear / LogSoftMax.
  // merge_head: the head launch also forms alpha / indicators / VBAR, sums the MLP GEMM's split-K slabs itself (no
  // reduce launch between them) and, with AttnDims::dlogp_early, runs the head's backward.
  int fwd_head(bool merge_head) {
    const int S = d.S, rows = d.B * d.T;
    if (d.dropout > 0.f) {
      hipLaunchKernelGGL(dec_dropout_fwd, dim3(512), dim3(256), 0, st, k, d.dropout, d.dropout_seed,
                         d.dropout_seed_dev, d.dropout_mask);
      S2S_CHECK_HIP(hipGetLastError());
    }
    {
      GemmDeferred dr{};
      GemmDeferReduce scope(merge_head && g_head_sums_slabs ? &dr : nullptr);
      S2S_TRY(gemm1(st, false, true, rows, d.M * d.K, S + d.A, 1.f, k.VV, S + d.A, k.P.Wm, S + d.A, 0.f, k.U,
                    (long)d.M * d.K, k.P.bm, gws));
      if (dr.splits > 1) { k.UP = dr.part; k.UPS = dr.splits; k.UPMN = dr.mn; }
      decide("dec.head_sums_slabs", dr.splits > 1);  // the head launch below really has slabs to sum
    }
    decide("dec.merged_head", merge_head);
    const bool hb = merge_head && attn_head_bwd_fused(d, r);
    decide("dec.head_bwd_fused", hb);
    k.dlogp = hb ? d.dlogp_early : nullptr;
    if (merge_head)
      hipLaunchKernelGGL(dec_xcd_alpha_vbar_head, dim3(d.T * d.B + ((d.Sc + 63) / 64) * d.B + (rows + 3) / 4),
                         dim3(256), 4 * (d.M + (hb ? d.O : 0)) * sizeof(float), st, k, x, rows);
    else
      hipLaunchKernelGGL(dec_mlp_head, dim3((rows + 3) / 4), dim3(256), 4 * d.M * sizeof(float), st, k, rows);
    S2S_CHECK_HIP(hipGetLastError());
    return 0;
  }
  // ---- backward, what every path starts from: DV = d[s_t; c_t] of all rows -- the caller's rows (external
  // decoder_mlp) or the MLP backward (the head's half unless the forward's head launch ran it), then the dropout mask.
  int bwd_mlp(const float* dlogp) {
    const int S = d.S, A = d.A, Mk = d.M * d.K, rows = d.B * d.T;
    if (d.ext) {  // dlogp holds d[s_t; c_t] (B*T, S+A)
      S2S_TRY(copy2d_f32(st, dlogp, S + A, k.DV, S + A, rows, S + A, false));
    } else {
      if (attn_head_bwd_fused(d, r)) {
        S2S_REQUIRE(dlogp == d.dlogp_early, "attn: dlogp_early differs from the backward's dlogp");
      } else {
        hipLaunchKernelGGL(dec_mlp_head_bwd, dim3((rows + 3) / 4), dim3(256), 4 * d.O * sizeof(float), st, k, rows);
        S2S_CHECK_HIP(hipGetLastError());
      }
      // dV = dU Wm  ->  [ds_mlp | dc_mlp]
      S2S_TRY(gemm1(st, false, false, rows, S + A, Mk, 1.f, k.DU, Mk, k.P.Wm, S + A, 0.f, k.DV, S + A, nullptr, gws));
    }
    if (d.dropout > 0.f) {
      hipLaunchKernelGGL(dec_dropout_bwd, dim3(512), dim3(256), 0, st, k);
      S2S_CHECK_HIP(hipGetLastError());
    }
    return 0;
  }
  // ---- backward, persist and per-step paths only (the XCD-local kernels write DVH / DWEACC whole and take their
  // layouts from the prologue): zeroed DVH / DWEACC, the packed transposes; folded, WDC^T = Wc^T Wd_c^T in WcT's place.
  int bwd_steps_operands() {
    const AttnParams& P = k.P;
    const int S = d.S, A = d.A, Sc = d.Sc;
    S2S_TRY(zero_async(st, k.DVH, sizeof(float) * (size_t)d.B * d.L * Sc));
    S2S_TRY(zero_async(st, k.DWEACC, sizeof(float) * (size_t)d.B * k.NCH * Sc));
    if (d.lstm) {  // GT = LW^T in the gate gradients' gate-major order
      hipLaunchKernelGGL(dec_lstm_gt, dim3(512), dim3(256), 0, st, k);
      S2S_CHECK_HIP(hipGetLastError());
    } else {
      S2S_TRY(transpose_f32(st, P.Wh, 2L * S, S, S, k.WhT, S));          // WhT[k][n] = Wh[n][k], k < S
      S2S_TRY(transpose_f32(st, P.Wz, 2L * S, S, 2 * S, k.GT, 3L * S));   // GT[c][n]      = Wz[n][c]
      S2S_TRY(transpose_f32(st, P.Wr, 2L * S, S, 2 * S, k.GT + S, 3L * S));
      S2S_TRY(transpose_f32(st, P.Wh, 2L * S, S, 2 * S, k.GT + 2 * S, 3L * S));
      // the h-half of Wh reaches ds_{t-1} through dq = Wh[:, :S]^T da_h (K2), not through GT
      hipLaunchKernelGGL(fill2d_kernel, dim3(64), dim3(256), 0, st, k.GT + 2 * S, 3L * S, S, S, 0.f);
    }
    if (!r.fold) {
      S2S_TRY(transpose_f32(st, P.Wd, 2L * S, S, 2 * S, k.WdT, S));
      S2S_TRY(transpose_f32(st, P.Wc, A, S, A, k.WcT, S));
    }
    S2S_TRY(transpose_f32(st, P.Ws, S, Sc, S, k.WsT, Sc));
    if (r.fold) {
      WgradPrecision wp;
      S2S_TRY(gemm1(st, true, true, A, S, S, 1.f, P.Wc, A, P.Wd, 2L * S, 0.f, k.WcT, S, nullptr, gws));
    }
    return 0;
  }
  // ---- backward, per-step launches.  Expects bwd_steps_operands and bwd_mlp.  T steps in reverse (folded: DCY by one
  // GEMM after them).  Writes no dh: attn_bwd_core finishes it from DC (alpha^T dc, beta 0 when not accumulating) and
  // DVH.  persist_fallback as in fwd_steps.
  int bwd_steps(bool persist_fallback) {
    const int B = d.B, S = d.S, A = d.A, Sc = d.Sc, rows = B * d.T, bt = (B + 15) / 16;
    hipLaunchKernelGGL(dec_bwd_init, dim3((B * S + 255) / 256), dim3(256), 0, st, k);
    // dec_b6_attn<true>'s dZ rows, staged taps and alpha halo
    const size_t b6_lds = d.hf > 0 ? sizeof(float) * ((LC + (size_t)d.hk) * Sc + LC + kMaxHybK) : 0;
    if (b6_lds > 32 * 1024)
      S2S_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dec_b6_attn<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)b6_lds));
    if (d.hf > 0) {
      S2S_TRY(zero_async(st, k.QA, sizeof(float) * 2 * (size_t)B * d.L * d.hk));
      S2S_TRY(zero_async(st, k.PDG, sizeof(float) * (size_t)B * k.NCH * d.hk * Sc));
    }
    ProfScope ps(st, "dec_bwd_steps", 0.0, 0.0);
    record_dec_launch(false, kPathSteps, r.xp, x, -1);
    if (persist_fallback) S2S_TRY(launch_sync_prep(st, k.bsync, 256, nullptr, k.bhdr));
    for (int t = d.T - 1; t >= 0; --t) {
      k.t = t;
      if (d.lstm) {
        hipLaunchKernelGGL(dec_b3_lstm, dim3(2 * S / 16, bt), dim3(512), 0, st, k);
      } else {
        hipLaunchKernelGGL(dec_b2_gru1, dim3(S / 16, bt), dim3(256), 0, st, k);
        hipLaunchKernelGGL(dec_b3_gru2, dim3(2 * S / 16, bt), dim3(256), 0, st, k);
      }
      if (r.fold) {
        hipLaunchKernelGGL(dec_b45_fold, dim3(A / 16, bt), dim3(512), 0, st, k, k.WcT);
      } else {
        hipLaunchKernelGGL(dec_b4_wd, dim3(2 * S / 16, bt), dim3(256), 0, st, k);
        hipLaunchKernelGGL(dec_b5_wc, dim3(A / 16, bt), dim3(256), 0, st, k);
      }
      if (d.hf > 0) hipLaunchKernelGGL(dec_b6_attn<true>, dim3(k.NCH, B), dim3(512), b6_lds, st, k);
      else hipLaunchKernelGGL(dec_b6_attn<false>, dim3(k.NCH, B), dim3(256), 0, st, k);
      hipLaunchKernelGGL(dec_b8_ws, dim3(S / 16, bt), dim3(256), 0, st, k);
    }
    S2S_CHECK_HIP(hipGetLastError());
    // [dc_in | dy_in] rows for the weight gradients (the folded steps never formed them): DCY = DD Wd
    if (r.fold)
      S2S_TRY(gemm1(st, false, false, rows, 2 * S, S, 1.f, k.DD, S, k.P.Wd, 2L * S, 0.f, k.DCY, 2L * S, nullptr, gws));
    return 0;
  }
  // ---- backward, the 7-seam persistent kernel.  Expects bwd_steps_operands, bwd_mlp and a dh it can add to (zeroed by
  // attn_bwd_core if not accumulating): it adds alpha^T dc to k.dh step by step (dh_has_dc); attn_bwd_core adds dVh V.
  int bwd_persist() {
    const int pgrid = kDecWG * ((d.B + 15) / 16);
    const PersistLaunch pb = pick_dec(false, r.pvar, d, pgrid);
    if (!pb.fn) return bwd_steps(true);  // the route says persist, the launch has no candidate
    dh_has_dc = true;
    S2S_TRY(launch_sync_prep(st, k.bsync, k.bsync_bytes, nullptr, k.bhdr));
    ProfScope ps(st, "dec_bwd_persist", 0.0, 0.0);
    record_dec_launch(false, kPathPersist, r.xp, x, pb.res);
    S2S_TRY(launch_persist(pb, pgrid, st, k));
    S2S_CHECK_HIP(hipGetLastError());
    return 0;
  }
  // ---- backward, the XCD-local kernels.  Expects bwd_mlp, the prologue's operands and, when split, the forward's
  // side-stream results (ev[2]).  One launch for all T steps, then dVh / dwe (dec_xcd_dvh; on the side stream if split:
  // ev[4]).  Writes no dh: attn_bwd_core finishes it from DC (beta 0 when not accumulating) and DVH, or defers both.
  int bwd_xcd() {
    set_plan();
    if (!d.syncs_in_prologue) S2S_TRY(launch_sync_prep(st, k.bsync, k.bsync_bytes, nullptr, k.bhdr));
    if (side) S2S_CHECK_HIP(hipStreamWaitEvent(st, ev[2], 0));  // VBAR, ALPHA, IND from the forward's side stream
    {
      ProfScope ps(st, lstm_xcd() ? "dec_bwd_xcd_lstm" : "dec_bwd_xcd", dec_flops(d, true),
                   8.0 * d.T * d.B * d.L * (double)(d.Sc + d.A));
      record_dec_launch(false, r.path, r.xp, x, -1);
      S2S_TRY(launch_chains(false));
    }
    if (side) {
      S2S_CHECK_HIP(hipEventRecord(ev[3], st));
      S2S_CHECK_HIP(hipStreamWaitEvent(side, ev[3], 0));
    }
    const void* fn = d.hf > 0 ? (const void*)dec_xcd_dvh_hyb : (const void*)dec_xcd_dvh;
    const size_t lds = d.hf > 0 ? dec_xcd_dvh_hyb_lds(d.T) : dec_xcd_dvh_lds(d.T);
    if (lds > 64 * 1024) S2S_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (d.hf > 0)  // the location features inside the tanh terms (dec_xcd_lstm.inc)
      hipLaunchKernelGGL(dec_xcd_dvh_hyb, dim3((d.Sc + 63) / 64, k.NCH, d.B), dim3(256), lds, side ? side : st, k, x);
    else
      hipLaunchKernelGGL(dec_xcd_dvh, dim3((d.Sc + 63) / 64, (d.L + kDvhF - 1) / kDvhF, d.B), dim3(256), lds,
                         side ? side : st, k, x);
    S2S_CHECK_HIP(hipGetLastError());
    if (side) S2S_CHECK_HIP(hipEventRecord(ev[4], side));
    return 0;
  }
};

// the decoder launches of d's path hand off through the fsync / bsync regions of `scratch` (the XCD-local or
// the persistent kernels; the per-step path has none): their headers, for the caller's harvest
int attn_sync_regions(const AttnDims& d, void* saved, void* scratch, void** fwd, void** bwd) {
  *fwd = *bwd = nullptr;
  if (dec_route(d).path == kPathSteps) return 0;
  AttnK k{};
  carve(d, &k, static_cast<char*>(saved), static_cast<char*>(scratch));
  *fwd = k.fhdr;
  *bwd = k.bhdr;
  return 2;
}

int attn_fwd_prologue(hipStream_t st, const AttnDims& d, const int* labels, const AttnParams& P, void* saved,
                      void* scratch) {
  DecCall c(st, d, saved, scratch);
  if (!c.r.xcd()) return 0;
  c.k.P = P; c.k.labels = labels;
  S2S_TRY(c.prologue());
  if (d.syncs_in_prologue) {  // both decoder launches' sync regions, off the decoder's critical path
    S2S_TRY(launch_sync_prep(st, c.k.fsync, c.k.fsync_bytes, nullptr, c.k.fhdr));
    S2S_TRY(launch_sync_prep(st, c.k.bsync, c.k.bsync_bytes, nullptr, c.k.bhdr));
  }
  return 0;
}

int attn_fwd(hipStream_t st, const AttnDims& d, const float* h, const int* labels, const AttnParams& P, float* logp,
             void* saved, void* scratch, size_t scratch_bytes, bool prologue_done, hipStream_t side, hipEvent_t* ev) {
  S2S_TRY(attn_check_dims(d));
  S2S_REQUIRE(scratch_bytes >= attn_scratch_bytes(d), "attn: scratch too small");
  S2S_REQUIRE(!d.dlogp_early || !side, "attn: dlogp_early (the head's backward in the forward) takes no side stream");
  DecCall c(st, d, saved, scratch, side, ev);
  c.k.P = P; c.k.h = h; c.k.labels = labels; c.k.logp = logp; c.k.stamps = g_dec_stamps[0];
  // Vh = h V^T  (TemporalConvolutionZeroBias(A, Sc, 1), Attention.lua:44)
  S2S_TRY(gemm1(st, false, true, d.B * d.L, d.Sc, d.A, 1.f, h, d.A, P.V, d.A, 0.f, c.k.Vh, d.Sc, nullptr, c.gws));
  const bool merge_head = merged_head(d, c.r, side);  // dec_xcd_alpha_vbar_head
  switch (c.r.path) {
    case kPathSteps: S2S_TRY(c.fwd_steps(false)); break;
    case kPathPersist: S2S_TRY(c.fwd_persist()); break;
    default: S2S_TRY(c.fwd_xcd(prologue_done, merge_head));  // kPathXcd, kPathXcdLstm
  }
  if (d.ext) return 0;  // external decoder_mlp: the caller runs it on the saved VV rows
  return c.fwd_head(merge_head);
}

int attn_dh_gemms(hipStream_t st, const AttnDhTerms& t, float* dh, int accumulate_dh, hipEvent_t dvh_ready) {
  const int B = t.B, L = t.L, T = t.T, A = t.A;
  const GemmWs gws = t.gws;
  // dh_l (+)= sum_t alpha_{t,l} dc_t  (one GEMM per utterance: alpha_b^T (L x T) . dc_b (T x A))
  for (int b0 = 0; b0 < B; b0 += kMaxGemmBatch) {
    GemmProblem pr[kMaxGemmBatch];
    const int nb = std::min(kMaxGemmBatch, B - b0);
    for (int i = 0; i < nb; ++i) {
      const long b = b0 + i;
      pr[i] = GemmProblem{t.alpha + b * T * L, t.dc + b * T * A, dh + b * L * A, nullptr, L, A, A, L, A, T,
                          1.f, accumulate_dh ? 1.f : 0.f};
    }
    S2S_TRY(gemm_f32(st, pr, nb, true, false, gws));
  }
  if (dvh_ready) S2S_CHECK_HIP(hipStreamWaitEvent(st, dvh_ready, 0));
  // dh += dVh V   (Vh = h V^T)
  return gemm1(st, false, false, B * L, A, t.Sc, 1.f, t.dvh, t.Sc, t.V, A, 1.f, dh, A, nullptr, gws);
}

int attn_bwd_core(hipStream_t st, const AttnDims& d, const float* h, const int* labels, const AttnParams& P,
                  const void* saved, const float* dlogp, float* dh, int accumulate_dh, void* scratch,
                  size_t scratch_bytes, hipStream_t side, hipEvent_t* ev, AttnDhTerms* defer_dh) {
  if (defer_dh) *defer_dh = AttnDhTerms{};
  S2S_TRY(attn_check_dims(d));
  S2S_REQUIRE(scratch_bytes >= attn_scratch_bytes(d), "attn: scratch too small");
  DecCall c(st, d, saved, scratch, side, ev);
  AttnK& k = c.k;
  k.P = P; k.h = h; k.labels = labels; k.dlogp = dlogp; k.dh = dh; k.lddh = d.A; k.stamps = g_dec_stamps[1];
  const bool xcd = c.r.xcd();
  // the persistent kernels accumulate dh in place (every other path: attn_dh_gemms below, beta 0 if not accumulating)
  const bool zero_dh = !accumulate_dh && c.r.path == kPathPersist;
  if (zero_dh) S2S_TRY(zero_async(st, dh, sizeof(float) * (size_t)d.B * d.L * d.A));
  if (!xcd) S2S_TRY(c.bwd_steps_operands());
  S2S_TRY(c.bwd_mlp(dlogp));
  switch (c.r.path) {
    case kPathSteps: S2S_TRY(c.bwd_steps(false)); break;
    case kPathPersist: S2S_TRY(c.bwd_persist()); break;
    default: S2S_TRY(c.bwd_xcd());  // kPathXcd, kPathXcdLstm
  }
  // ---- dh is finished here, for every path: dh (+)= sum_t alpha_t^T dc_t (per utterance) + dVh V  (Vh = h V^T)
  if (c.dh_has_dc)  // (the persistent kernel)
    return gemm1(st, false, false, d.B * d.L, d.A, d.Sc, 1.f, k.DVH, d.Sc, P.V, d.A, 1.f, dh, d.A, nullptr, c.gws);
  const AttnDhTerms terms{k.ALPHA, k.DC /* = XArgs::DCS */, k.DVH, P.V, d.B, d.L, d.T, d.A, d.Sc, c.gws};
  if (xcd && defer_dh && !accumulate_dh) {  // the caller fuses both terms into the encoder BPTT launch
    if (side) S2S_CHECK_HIP(hipStreamWaitEvent(st, ev[4], 0));
    *defer_dh = terms;
    return 0;
  }
  return attn_dh_gemms(st, terms, dh, accumulate_dh, xcd && side ? ev[4] : nullptr);
}

// Weight gradients: one GEMM per parameter over all B*T rows (accumulate, alpha = scale), then
// the bias column sums.  Reads only the saved buffer and attn_bwd_core's scratch, so the model
// step runs it on a side stream beside the encoder BPTT.
int attn_bwd_wgrad(hipStream_t st, const AttnDims& d, const float* h, const int* labels, const AttnParams& P,
                   const void* saved, const AttnGrads& G, float scale, void* scratch) {
  WgradPrecision wp;
  DecCall c(st, d, saved, scratch);
  AttnK& k = c.k;
  const GemmWs gws = c.gws;  // (its GEMM and column-sum launches reuse the slabs in stream order)
  k.labels = labels;
  const int B = d.B, L = d.L, T = d.T, S = d.S, A = d.A, Sc = d.Sc, O = d.O, Mk = d.M * d.K;
  const int rows = B * T;
  hipLaunchKernelGGL(dec_onehot_prev, dim3(256), dim3(256), 0, st, k);
  S2S_CHECK_HIP(hipGetLastError());
  if (c.r.xcd()) {
    // the XCD-local loops folded c -> c_in -> d away: recompute c_in, d = HX[:, S:] (the cell's input; the GRU also
    // reads it from RHX), dd = dGA WXD (the gates' x-weights: 3 GRU / 4 LSTM blocks) and [dc_in | dy_in] = dd Wd for
    // the weight gradients, all B*T rows at once
    const int NG = d.lstm ? 4 : 3;
    S2S_TRY(gemm1(st, false, true, rows, S, A, 1.f, k.C, A, P.Wc, A, 0.f, k.CY, 2L * S, P.bc, gws));
    S2S_TRY(gemm1(st, false, true, rows, S, 2 * S, 1.f, k.CY, 2L * S, P.Wd, 2L * S, 0.f, k.HX + S, 2L * S, P.bd, gws));
    if (!d.lstm) S2S_TRY(copy2d_f32(st, k.HX + S, 2L * S, k.RHX + S, 2L * S, rows, S, false));
    const float* wxd = d.lstm ? c.y.WXD4 : c.x.WXD;
    S2S_TRY(gemm1(st, false, false, rows, S, NG * S, 1.f, k.DGA, (long)NG * S, wxd, S, 0.f, k.DD, S, nullptr, gws));
    S2S_TRY(gemm1(st, false, false, rows, 2 * S, S, 1.f, k.DD, S, P.Wd, 2L * S, 0.f, k.DCY, 2L * S, nullptr, gws));
  }
  {
    GemmProblem pr[16];
    int n = 0;
    if (!d.ext) {
      pr[n++] = GemmProblem{k.DO, k.MM, G.Wo, nullptr, O, d.M, d.M, O, d.M, rows, scale, 1.f};
      pr[n++] = GemmProblem{k.DU, k.VV, G.Wm, nullptr, Mk, S + A, S + A, Mk, S + A, rows, scale, 1.f};
    }
    if (d.lstm) {  // all four gates' [Wqh | Wqx] grads at once, staged in LDW (scattered below)
      pr[n++] = GemmProblem{k.DGA, k.HX, k.LDW, nullptr, 4L * S, 2L * S, 2L * S, 4 * S, 2 * S, rows, scale, 0.f};
    } else {
      pr[n++] = GemmProblem{k.DGA, k.HX, G.Wz, nullptr, 3L * S, 2L * S, 2L * S, S, 2 * S, rows, scale, 1.f};
      pr[n++] = GemmProblem{k.DGA + S, k.HX, G.Wr, nullptr, 3L * S, 2L * S, 2L * S, S, 2 * S, rows, scale, 1.f};
      pr[n++] = GemmProblem{k.DGA + 2 * S, k.RHX, G.Wh, nullptr, 3L * S, 2L * S, 2L * S, S, 2 * S, rows, scale,
                            1.f};
    }
    pr[n++] = GemmProblem{k.DD, k.CY, G.Wd, nullptr, S, 2L * S, 2L * S, S, 2 * S, rows, scale, 1.f};
    pr[n++] = GemmProblem{k.DCY, k.C, G.Wc, nullptr, 2L * S, A, A, S, A, rows, scale, 1.f};
    pr[n++] = GemmProblem{k.DCY + S, k.YP, G.Wy, nullptr, 2L * S, O, O, S, O, rows, scale, 1.f};
    pr[n++] = GemmProblem{k.DWS, k.HX, G.Ws, nullptr, Sc, 2L * S, S, Sc, S, rows, scale, 1.f};
    pr[n++] = GemmProblem{k.DVH, h, G.V, nullptr, Sc, A, A, Sc, A, B * L, scale, 1.f};
    S2S_TRY(gemm_f32(st, pr, n, true, false, gws));
  }
  if (!d.ext) {
    S2S_TRY(colsum_f32(st, k.DO, O, rows, O, scale, 1.f, G.bo, gws));
    S2S_TRY(colsum_f32(st, k.DU, Mk, rows, Mk, scale, 1.f, G.bm, gws));
  }
  S2S_TRY(colsum_f32(st, k.DD, S, rows, S, scale, 1.f, G.bd, gws));
  if (d.lstm) {
    ColsumOut outs[4];
    // LSTM.lua:25-29: Linear(S,S)(x) + Linear(S,S)(h), both with bias: the four gates' Wqx / Wqh blocks of LDW added
    // into their tensors in one launch (eight copy launches before)
    hipLaunchKernelGGL(lstm_dw_scatter, dim3(1024), dim3(256), 0, st, k.LDW, S, G);
    S2S_CHECK_HIP(hipGetLastError());
    for (int q = 0; q < 4; ++q) outs[q] = ColsumOut{q * S, S, {G.lstm[4 * q + 1], G.lstm[4 * q + 3], nullptr}, 2};  // bqx, bqh
    S2S_TRY(colsum_scatter_f32(st, k.DGA, 4L * S, rows, 4 * S, scale, outs, 4, gws));
  }
  {
    const ColsumOut outs[2] = {{0, S, {G.bc, nullptr, nullptr}, 1}, {S, S, {G.by, nullptr, nullptr}, 1}};
    S2S_TRY(colsum_scatter_f32(st, k.DCY, 2L * S, rows, 2 * S, scale, outs, 2, gws));
  }
  S2S_TRY(colsum_f32(st, k.DWS, Sc, rows, Sc, scale, 1.f, G.bs, gws));
  S2S_TRY(colsum_f32(st, k.DWEACC, Sc, B * k.NCH, Sc, scale, 1.f, G.we, gws));
  if (d.hf > 0) {  // hybrid features: dG (sum over utterances, chunks; steps summed in the loop), dcu = sum dws
    k.P = P;
    if (c.r.path == kPathXcdLstm)  // the XCD-local chunks' partials (dec_xcd_lstm_bwd)
      S2S_TRY(colsum_f32(st, c.y.PDG, (long)d.hk * Sc, B * c.r.xp.NCH, d.hk * Sc, 1.f, 0.f, k.DGT, gws));
    else
      S2S_TRY(colsum_f32(st, k.PDG, (long)d.hk * Sc, B * k.NCH, d.hk * Sc, 1.f, 0.f, k.DGT, gws));
    S2S_TRY(colsum_f32(st, k.DWS, Sc, rows, Sc, 1.f, 0.f, k.DCU, gws));
    const int n = Sc * d.hf + d.hf * d.hk + d.hf;
    hipLaunchKernelGGL(dec_hyb_wgrad, dim3((n + 3) / 4), dim3(256), 0, st, k, G, scale);
    S2S_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

int attn_bwd(hipStream_t st, const AttnDims& d, const float* h, const int* labels, const AttnParams& P,
             const void* saved, const float* dlogp, float* dh, int accumulate_dh, const AttnGrads& G, float scale,
             void* scratch, size_t scratch_bytes) {
  S2S_TRY(attn_bwd_core(st, d, h, labels, P, saved, dlogp, dh, accumulate_dh, scratch, scratch_bytes));
  return attn_bwd_wgrad(st, d, h, labels, P, saved, G, scale, scratch);
}

#include "beam.inc"

int set_device_u64(hipStream_t st, unsigned long long* p, unsigned long long v) {
  hipLaunchKernelGGL(set_u64_kernel, dim3(1), dim3(64), 0, st, p, v);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace s2s

// Diagnostic (not part of the C ABI header): device buffers of uint64 s_memrealtime stamps the persistent
// decoder kernels fill at phase ends -- (grid, T, 8) for attn_persist.inc, (chains * 32, T, 16) for
// dec_xcd.inc (tools/xdec_stamps.py, tools/xdec_substamps.py); nullptr turns it off.
// diagnostic: 0 forces write-through (sc1) hand-offs in every XCD-local decoder chain
extern "C" void s2s_debug_dec_local(int allow) { s2s::g_dec_allow_local = allow; }
// diagnostic: 1 sends content attention's beam search down the replicated path too (A/B arm; set between searches)
extern "C" void s2s_debug_beam_replicate(int on) { s2s::g_beam_replicate = on ? 1 : 0; }
extern "C" void s2s_debug_merge_alpha_head(int on) { s2s::g_merge_alpha_head = on; }
// diagnostic: the merged MLP head sums the MLP GEMM's split-K slabs (1) or a reduce launch runs in front of it (0)
extern "C" void s2s_debug_head_sums_slabs(int on) { s2s::g_head_sums_slabs = on; }
extern "C" void s2s_debug_dec_r4(int on) { s2s::g_dec_r4 = on; }
extern "C" void s2s_debug_dvh_wide(int on) {
  const int v = on ? 1 : 0;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(s2s::g_dvh_force_wide), &v, sizeof(int));
}
extern "C" void s2s_debug_dec_mode(int m) { s2s::g_dec_mode_force = m; }
extern "C" void s2s_debug_dec_pf(int on) {  // 0: the XCD decoder's per-term attention form everywhere (A/B, tests)
  const int v = on ? 1 : 0;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(s2s::g_dec_pf), &v, sizeof(int));
  s2s::g_dec_pf_host = v;
}
extern "C" int s2s_debug_dec_stamps(void* fwd, void* bwd) {
  s2s::g_dec_stamps[0] = static_cast<unsigned long long*>(fwd);
  s2s::g_dec_stamps[1] = static_cast<unsigned long long*>(bwd);
  return 0;
}
