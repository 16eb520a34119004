// C-ABI surface of libs2s_hip.so (include/s2s_hip.h): the error string, the context, argument checking of the
// module-level calls, the optimizer and weight-noise calls, and RCCL data-parallel gradient sums.  The model-level
// training step is model_step.cpp, the flat parameter layout model_layout.cpp, live kernel timing prof.cpp, the
// s2s_debug_* entry points capi_debug.cpp.
#include <cstring>
#include <string>

#include "ctx.h"
#include "frontend.h"
#include "gru.h"
#include "handoff.h"
#include "lstm.h"

namespace s2s {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* get_error() { return g_err.c_str(); }

// the stream a module-level backward issues its parameter gradients on: `st`, or the context's side stream forked
// from `st` here when the caller set s2s_ctx_set_wgrad_overlap (joined by s2s_ctx_join_wgrad)
int wgrad_stream(s2s_ctx* ctx, hipStream_t st, hipStream_t* out) {
  *out = st;
  if (!ctx->wgrad_overlap || !ctx->wside || !ctx->wev || ctx->wside == st) return 0;
  S2S_CHECK_HIP(hipEventRecord(ctx->wev, st));
  S2S_CHECK_HIP(hipStreamWaitEvent(ctx->wside, ctx->wev, 0));
  *out = ctx->wside;
  return 0;
}

// every compute entry point starts here: the device, the context's GEMM precision for this call, and the
// context's failure status -- a persistent launch of an earlier call that timed out left wrong results, so
// every later call fails until the caller has seen it (s2s_ctx_status with clear = 1); Torch's error()
int set_device(s2s_ctx* ctx) {
  S2S_REQUIRE(ctx != nullptr, "null context");
  if (ctx->status_host) {
    const unsigned t = __atomic_load_n(ctx->status_host, __ATOMIC_ACQUIRE);
    const unsigned a = __atomic_load_n(ctx->status_host + 1, __ATOMIC_ACQUIRE);
    S2S_REQUIRE(t == 0u && a == 0u,
                std::string("a persistent launch of an earlier call failed (") +
                    (t ? "hand-off wait timed out" : "launch started on an aborted sync region") +
                    "): its outputs and gradients are invalid; s2s_ctx_status(ctx, stream, &st, 1) clears it");
  }
  S2S_CHECK_HIP(hipSetDevice(ctx->device));
  set_gemm_precision(ctx->precision == S2S_PREC_FP32 ? kGemmF32 : kGemmBf16);
  set_wgrad_bf16(ctx->precision == S2S_PREC_BF16_ALL);
  set_gemm_stage(&ctx->lt);
  return 0;
}

AttnDims to_attn(const s2s_attn_dims* d) {
  AttnDims a{d->B, d->L, d->T, d->annotationDepth, d->scoreDepth, d->stateDepth, d->outputDepth, d->mlpDepth,
             d->maxoutWindow, d->penalty, d->dropout, d->dropout_seed, d->dropout_mask};
  a.hk = d->hybridAttendFilterSize;
  a.hf = d->hybridAttendFeatureMaps;
  a.ext = d->external_mlp ? 1 : 0;
  a.lstm = d->decoder_lstm ? 1 : 0;
  a.flen = d->frame_lengths;
  a.tlen = d->label_lengths;
  a.share_hybrid = d->beam_share_hybrid ? 1 : 0;
  return a;
}

}  // namespace s2s

using namespace s2s;

namespace {

int attn_nparams(const s2s_attn_dims* d) {
  if (d->decoder_lstm) return S2S_ATTN_NPARAMS_LSTM;
  return d->hybridAttendFeatureMaps > 0 ? S2S_ATTN_NPARAMS_HYBRID : S2S_ATTN_NPARAMS;
}
// parameter slots a call may leave NULL: the fused MLP's with an external decoder_mlp, the GRU's with a
// decoder LSTM, the hybrid ones without hybrid features
bool attn_param_optional(const s2s_attn_dims* d, int i) {
  if (d->external_mlp && i >= 13 && i <= 16) return true;
  if (d->decoder_lstm && i >= 10 && i <= 12) return true;
  if (d->hybridAttendFeatureMaps <= 0 && i >= 17 && i <= 19) return true;
  return false;
}

}  // namespace

// ================================================================== C ABI
extern "C" {

int s2s_version(void) { return 1; }

const char* s2s_last_error(void) { return s2s::get_error(); }

int s2s_ctx_create(int device, s2s_ctx** out) {
  S2S_REQUIRE(out != nullptr, "null out");
  int n = 0;
  S2S_CHECK_HIP(hipGetDeviceCount(&n));
  S2S_REQUIRE(device >= 0 && device < n, "device index out of range");
  S2S_CHECK_HIP(hipSetDevice(device));
  auto* c = new s2s_ctx();
  c->device = device;
  if (hipHostMalloc(reinterpret_cast<void**>(&c->status_host), 64, hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void**>(&c->status_dev), c->status_host, 0) != hipSuccess) {
    if (c->status_host) (void)hipHostFree(c->status_host);
    delete c;
    S2S_REQUIRE(false, "ctx: host-coherent status word allocation failed");
  }
  if (c->status_host) std::memset(c->status_host, 0, 64);
  // (the side stream at the lowest queue priority measured no change)
  if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess) {
    c->side = nullptr;
  }
  for (auto& e : c->ev)
    if (c->side && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      (void)hipStreamDestroy(c->side);
      c->side = nullptr;
    }
  if (hipStreamCreateWithFlags(&c->wside, hipStreamNonBlocking) != hipSuccess) c->wside = nullptr;
  if (c->wside && hipEventCreateWithFlags(&c->wev, hipEventDisableTiming) != hipSuccess) c->wev = nullptr;
  *out = c;
  return 0;
}

void s2s_ctx_destroy(s2s_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (auto& g : ctx->graphs) (void)drop_graph(ctx, g);
  ctx->graphs.clear();
  if (ctx->seed_dev) (void)hipFree(ctx->seed_dev);
  s2s::gemm_stage_free(&ctx->lt);
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  for (auto& e : ctx->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->bev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->wev) (void)hipEventDestroy(ctx->wev);
  if (ctx->wside) (void)hipStreamDestroy(ctx->wside);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->status_host) (void)hipHostFree(ctx->status_host);
  delete ctx;
}

int s2s_ctx_set_flags(s2s_ctx* ctx, int flags) {
  S2S_REQUIRE(ctx != nullptr, "null context");
  ctx->flags = flags;
  return 0;
}

int s2s_ctx_set_wgrad_overlap(s2s_ctx* ctx, int on) {
  S2S_REQUIRE(ctx != nullptr, "null context");
  S2S_REQUIRE(!on || (ctx->wside && ctx->wev), "ctx: no stream for the parameter gradients");
  ctx->wgrad_overlap = on ? 1 : 0;
  return 0;
}

int s2s_ctx_join_wgrad(s2s_ctx* ctx, s2s_stream_t stream) {
  S2S_REQUIRE(ctx != nullptr, "null context");
  if (!ctx->wside || !ctx->wev || static_cast<hipStream_t>(stream) == ctx->wside) return 0;
  S2S_CHECK_HIP(hipSetDevice(ctx->device));
  S2S_CHECK_HIP(hipEventRecord(ctx->wev, ctx->wside));
  S2S_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), ctx->wev, 0));
  return 0;
}

s2s_stream_t s2s_ctx_side_stream(s2s_ctx* ctx) { return ctx ? static_cast<s2s_stream_t>(ctx->wside) : nullptr; }

int s2s_ctx_status(s2s_ctx* ctx, s2s_stream_t stream, int* status, int clear) {
  S2S_REQUIRE(ctx != nullptr && status != nullptr, "null argument");
  S2S_CHECK_HIP(hipSetDevice(ctx->device));
  S2S_CHECK_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  if (ctx->side) S2S_CHECK_HIP(hipStreamSynchronize(ctx->side));
  if (ctx->wside) S2S_CHECK_HIP(hipStreamSynchronize(ctx->wside));
  *status = 0;
  if (!ctx->status_host) return 0;
  *status = (__atomic_load_n(ctx->status_host, __ATOMIC_ACQUIRE) ? S2S_STATUS_HANDOFF_TIMEOUT : 0) |
            (__atomic_load_n(ctx->status_host + 1, __ATOMIC_ACQUIRE) ? S2S_STATUS_ABORTED_REGION : 0);
  if (clear)
    for (int i = 0; i < 16; ++i) __atomic_store_n(ctx->status_host + i, 0u, __ATOMIC_RELEASE);
  return 0;
}

int s2s_ctx_set_precision(s2s_ctx* ctx, int precision) {
  S2S_REQUIRE(ctx != nullptr, "null context");
  S2S_REQUIRE(precision == S2S_PREC_FP32 || precision == S2S_PREC_BF16_GEMM || precision == S2S_PREC_BF16_ALL,
              "unknown precision");
  ctx->precision = precision;
  return 0;
}

size_t s2s_gru_saved_bytes(int B, int L, int H) { return sizeof(float) * (size_t)B * L * 5 * H; }
size_t s2s_gru_scratch_bytes(int ndir, int B, int L, int D, int H) {
  return gru_layer_scratch_bytes(ndir, B, L, D, H);
}

static int fill_gru_io(GruLayerIO& io, int ndir, int B, int L, int D, int H, const int* reverse, const float* x,
                       long ldx, const float* const* W, float* const* y, long ldy, void* const* saved,
                       const int* lengths) {
  S2S_REQUIRE(ndir == 1 || ndir == 2, "gru: ndir must be 1 or 2");
  S2S_REQUIRE(reverse && x && W && saved, "gru: null argument");
  S2S_REQUIRE(ldx >= D, "gru: ldx < D");
  io.ndir = ndir; io.B = B; io.L = L; io.D = D; io.H = H; io.x = x; io.ldx = ldx; io.ldy = ldy;
  io.len = lengths;
  for (int d = 0; d < ndir; ++d) {
    for (int g = 0; g < 3; ++g) {
      io.W[d][g] = W[3 * d + g];
      S2S_REQUIRE(io.W[d][g] != nullptr, "gru: null weight");
    }
    io.reverse[d] = reverse[d] ? 1 : 0;
    io.y[d] = y ? y[d] : nullptr;
    io.saved[d] = static_cast<float*>(saved[d]);
    S2S_REQUIRE(io.saved[d] != nullptr, "gru: null saved buffer");
  }
  return 0;
}

int s2s_gru_fwd(s2s_ctx* ctx, s2s_stream_t stream, int ndir, int B, int L, int D, int H, const int* reverse,
                const float* x, long ldx, const float* const* W, float* const* y, long ldy, void* const* saved,
                const int* lengths, void* scratch, size_t scratch_bytes) {
  S2S_TRY(set_device(ctx));
  GruLayerIO io{};
  S2S_TRY(fill_gru_io(io, ndir, B, L, D, H, reverse, x, ldx, W, y, ldy, saved, lengths));
  S2S_REQUIRE(y != nullptr, "gru: null y");
  for (int d = 0; d < ndir; ++d) S2S_REQUIRE(y[d] != nullptr, "gru: null y");
  S2S_REQUIRE(ldy >= H, "gru: ldy < H");
  io.status = ctx->status_dev;
  return gru_layer_fwd(static_cast<hipStream_t>(stream), io, scratch, scratch_bytes);
}

int s2s_gru_bwd(s2s_ctx* ctx, s2s_stream_t stream, int ndir, int B, int L, int D, int H, const int* reverse,
                const float* x, long ldx, const float* const* W, void* const* saved, const float* const* dy,
                long lddy, float* dx, long lddx, int dx_accumulate, float* const* dW, float scale,
                const int* lengths, void* scratch, size_t scratch_bytes) {
  S2S_TRY(set_device(ctx));
  GruLayerIO io{};
  S2S_TRY(fill_gru_io(io, ndir, B, L, D, H, reverse, x, ldx, W, nullptr, H, saved, lengths));
  S2S_REQUIRE(dy && dW, "gru: null dy/dW");
  GruLayerGrad gr{};
  for (int d = 0; d < ndir; ++d) {
    gr.dy[d] = dy[d];
    S2S_REQUIRE(gr.dy[d] != nullptr, "gru: null dy");
    for (int g = 0; g < 3; ++g) {
      gr.dW[d][g] = dW[3 * d + g];
      S2S_REQUIRE(gr.dW[d][g] != nullptr, "gru: null dW");
    }
  }
  gr.lddy = lddy;
  gr.dx = dx;
  gr.lddx = lddx;
  gr.dx_accumulate = dx_accumulate;
  gr.scale = scale;
  io.status = ctx->status_dev;
  return gru_layer_bwd(static_cast<hipStream_t>(stream), io, gr, scratch, scratch_bytes);
}

size_t s2s_lstm_saved_bytes(int B, int L, int H) { return lstm_saved_bytes(B, L, H); }
size_t s2s_lstm_scratch_bytes(int ndir, int B, int L, int D, int H, int peepholes) {
  return lstm_scratch_bytes(ndir, B, L, D, H, peepholes);
}

static int fill_lstm_io(LstmLayerIO& io, int ndir, int B, int L, int D, int H, int peep, const int* reverse,
                        const float* x, long ldx, const float* const* W, float* const* y, long ldy,
                        void* const* saved) {
  S2S_REQUIRE(ndir == 1 || ndir == 2, "lstm: ndir must be 1 or 2");
  S2S_REQUIRE(reverse && x && W && saved, "lstm: null argument");
  S2S_REQUIRE(ldx >= D, "lstm: ldx < D");
  io.ndir = ndir; io.B = B; io.L = L; io.D = D; io.H = H; io.peep = peep ? 1 : 0;
  io.x = x; io.ldx = ldx; io.W = W; io.ldy = ldy;
  for (int d = 0; d < ndir; ++d) {
    for (int p = 0; p < lstm_nparams(io.peep); ++p) S2S_REQUIRE(W[d * lstm_nparams(io.peep) + p], "lstm: null weight");
    io.reverse[d] = reverse[d] ? 1 : 0;
    io.y[d] = y ? y[d] : nullptr;
    io.saved[d] = static_cast<float*>(saved[d]);
    S2S_REQUIRE(io.saved[d] != nullptr, "lstm: null saved buffer");
  }
  return 0;
}

int s2s_lstm_fwd(s2s_ctx* ctx, s2s_stream_t stream, int ndir, int B, int L, int D, int H, int peepholes,
                 const int* reverse, const float* x, long ldx, const float* const* W, float* const* y, long ldy,
                 void* const* saved, const int* lengths, void* scratch, size_t scratch_bytes) {
  S2S_TRY(set_device(ctx));
  LstmLayerIO io{};
  S2S_TRY(fill_lstm_io(io, ndir, B, L, D, H, peepholes, reverse, x, ldx, W, y, ldy, saved));
  io.len = lengths;
  S2S_REQUIRE(y != nullptr, "lstm: null y");
  for (int d = 0; d < ndir; ++d) S2S_REQUIRE(y[d] != nullptr, "lstm: null y");
  io.status = ctx->status_dev;
  return lstm_layer_fwd(static_cast<hipStream_t>(stream), io, scratch, scratch_bytes);
}

int s2s_lstm_bwd(s2s_ctx* ctx, s2s_stream_t stream, int ndir, int B, int L, int D, int H, int peepholes,
                 const int* reverse, const float* x, long ldx, const float* const* W, void* const* saved,
                 const float* const* dy, long lddy, float* dx, long lddx, int dx_accumulate, float* const* dW,
                 float scale, const int* lengths, void* scratch, size_t scratch_bytes) {
  S2S_TRY(set_device(ctx));
  LstmLayerIO io{};
  S2S_TRY(fill_lstm_io(io, ndir, B, L, D, H, peepholes, reverse, x, ldx, W, nullptr, H, saved));
  io.len = lengths;
  S2S_REQUIRE(dy && dW, "lstm: null dy/dW");
  LstmLayerGrad gr{};
  for (int d = 0; d < ndir; ++d) {
    gr.dy[d] = dy[d];
    S2S_REQUIRE(gr.dy[d] != nullptr, "lstm: null dy");
    for (int p = 0; p < lstm_nparams(io.peep); ++p)
      S2S_REQUIRE(dW[d * lstm_nparams(io.peep) + p], "lstm: null dW");
  }
  gr.lddy = lddy; gr.dx = dx; gr.lddx = lddx; gr.dx_accumulate = dx_accumulate; gr.dW = dW; gr.scale = scale;
  if (ctx->wgrad_overlap) {  // the parameter gradients beside the caller's next launches, forked once dA is final
    gr.wst = ctx->wside;
    gr.wev = ctx->wev;
  }
  io.status = ctx->status_dev;
  return lstm_layer_bwd(static_cast<hipStream_t>(stream), io, gr, scratch, scratch_bytes);
}

size_t s2s_attn_saved_bytes(const s2s_attn_dims* d) { return d ? attn_saved_bytes(to_attn(d)) : 0; }
size_t s2s_attn_scratch_bytes(const s2s_attn_dims* d) { return d ? attn_scratch_bytes(to_attn(d)) : 0; }
const float* s2s_attn_mlp_input(const s2s_attn_dims* d, const void* saved) {
  return d && saved ? attn_saved_mlp_input(to_attn(d), saved) : nullptr;
}
const float* s2s_attn_alpha(const s2s_attn_dims* d, const void* saved) {
  return d && saved ? attn_saved_alpha(to_attn(d), saved) : nullptr;
}
const float* s2s_attn_ws(const s2s_attn_dims* d, const void* saved) {
  return d && saved ? attn_saved_ws(to_attn(d), saved) : nullptr;
}
const float* s2s_attn_vh(const s2s_attn_dims* d, const void* saved) {
  return d && saved ? attn_saved_vh(to_attn(d), saved) : nullptr;
}
const float* s2s_attn_mono_ind(const s2s_attn_dims* d, const void* saved) {
  return d && saved ? attn_saved_mono_ind(to_attn(d), saved) : nullptr;
}
const int* s2s_attn_maxout_argmax(const s2s_attn_dims* d, const void* saved) {
  return d && saved ? attn_saved_maxout_argmax(to_attn(d), saved) : nullptr;
}
const float* s2s_attn_dropout_mask(const s2s_attn_dims* d, const void* saved) {
  return d && saved ? attn_saved_dropout_mask(to_attn(d), saved) : nullptr;
}

// the decoder's persistent launch of this call (which = 0 forward, 1 backward) -> the context's status
static int harvest_attn(s2s_ctx* ctx, s2s_stream_t stream, const AttnDims& ad, void* saved, void* scratch, int which) {
  void* r[2];
  if (attn_sync_regions(ad, saved, scratch, &r[0], &r[1]) == 0) return 0;
  return launch_sync_harvest(static_cast<hipStream_t>(stream), &r[which], 1, ctx->status_dev);
}

int s2s_attn_fwd(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, const float* h, const int* labels,
                 const float* const* params, float* logp, void* saved, void* scratch, size_t scratch_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && h && labels && params && (logp || d->external_mlp) && saved, "attn: null argument");
  AttnParams ap;
  const float** pp = reinterpret_cast<const float**>(&ap);
  for (int i = 0; i < attn_nparams(d); ++i) {
    pp[i] = params[i];
    S2S_REQUIRE(pp[i] != nullptr || attn_param_optional(d, i), "attn: null parameter");
  }
  const AttnDims ad = to_attn(d);
  S2S_TRY(attn_fwd(static_cast<hipStream_t>(stream), ad, h, labels, ap, logp, saved, scratch, scratch_bytes));
  return harvest_attn(ctx, stream, ad, saved, scratch, 0);
}

int s2s_attn_bwd(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, const float* h, const int* labels,
                 const float* const* params, const void* saved, const float* dlogp, float* dh, int dh_accumulate,
                 float* const* grads, float scale, void* scratch, size_t scratch_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && h && labels && params && saved && dlogp && dh && grads, "attn: null argument");
  AttnParams ap;
  AttnGrads ag;
  const float** pp = reinterpret_cast<const float**>(&ap);
  float** gp = reinterpret_cast<float**>(&ag);
  for (int i = 0; i < attn_nparams(d); ++i) {
    pp[i] = params[i];
    gp[i] = grads[i];
    S2S_REQUIRE((pp[i] != nullptr && gp[i] != nullptr) || attn_param_optional(d, i), "attn: null parameter/grad");
  }
  const AttnDims ad = to_attn(d);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  S2S_TRY(attn_bwd_core(st, ad, h, labels, ap, saved, dlogp, dh, dh_accumulate, scratch, scratch_bytes));
  // accGradParameters beside the caller's next launches (s2s_ctx_set_wgrad_overlap): it reads only saved and scratch
  hipStream_t wst;
  S2S_TRY(wgrad_stream(ctx, st, &wst));
  S2S_TRY(attn_bwd_wgrad(wst, ad, h, labels, ap, saved, ag, scale, scratch));
  return harvest_attn(ctx, stream, ad, const_cast<void*>(saved), scratch, 1);
}

size_t s2s_attn_beam_workspace_bytes(const s2s_attn_dims* d, int K, int maxseqlength) {
  if (!d || K < 1 || maxseqlength < 1) return 0;
  return attn_beam_workspace_bytes(to_attn(d), K, maxseqlength);
}

static int beam_params(const s2s_attn_dims* d, const float* const* params, AttnParams& ap) {
  S2S_REQUIRE(params, "beam search: null parameters");
  const float** pp = reinterpret_cast<const float**>(&ap);
  for (int i = 0; i < attn_nparams(d); ++i) {
    pp[i] = params[i];
    S2S_REQUIRE(pp[i] != nullptr || attn_param_optional(d, i), "beam search: null parameter");
  }
  return 0;
}

int s2s_attn_beam_search(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, const float* h,
                         const float* const* params, int eos, int K, int maxseqlength, int* out, int ldo, int* out_len,
                         float* out_score, void* workspace, size_t workspace_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && h && out && out_len && workspace, "beam search: null argument");
  AttnParams ap{};
  S2S_TRY(beam_params(d, params, ap));
  return attn_beam_search(static_cast<hipStream_t>(stream), to_attn(d), h, ap, eos, K, maxseqlength, nullptr, out,
                          ldo, out_len, out_score, workspace, workspace_bytes);
}

int s2s_attn_beam_search_ragged(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, const float* h,
                                const float* const* params, int eos, int K, int maxseqlength,
                                const int* maxseqlengths, int* out, int ldo, int* out_len, float* out_score,
                                void* workspace, size_t workspace_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && h && out && out_len && workspace, "beam search: null argument");
  AttnParams ap{};
  S2S_TRY(beam_params(d, params, ap));
  return attn_beam_search(static_cast<hipStream_t>(stream), to_attn(d), h, ap, eos, K, maxseqlength, maxseqlengths,
                          out, ldo, out_len, out_score, workspace, workspace_bytes);
}

int s2s_attn_beam_set_maxlens(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, int K, int maxseqlength,
                              const int* maxseqlengths, void* workspace) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && workspace && maxseqlengths, "beam search: null argument");
  return attn_beam_set_maxlens(static_cast<hipStream_t>(stream), to_attn(d), K, maxseqlength, maxseqlengths,
                               workspace);
}

int s2s_attn_beam_init(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, const float* h,
                       const float* const* params, int eos, int K, int maxseqlength, void* workspace,
                       size_t workspace_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && h && workspace, "beam search: null argument");
  AttnParams ap{};
  S2S_TRY(beam_params(d, params, ap));
  return attn_beam_init(static_cast<hipStream_t>(stream), to_attn(d), h, ap, eos, K, maxseqlength, workspace,
                        workspace_bytes);
}

int s2s_attn_beam_step(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, const float* const* params, int K,
                       int maxseqlength, int count, void* workspace, size_t workspace_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && workspace && count >= 0 && count <= maxseqlength, "beam search: bad step");
  AttnParams ap{};
  S2S_TRY(beam_params(d, params, ap));
  return attn_beam_step(static_cast<hipStream_t>(stream), to_attn(d), ap, K, maxseqlength, count, workspace,
                        workspace_bytes);
}

const float* s2s_attn_beam_mlp_input(const s2s_attn_dims* d, int K, int maxseqlength, void* workspace) {
  return d && workspace ? attn_beam_mlp_input(to_attn(d), K, maxseqlength, workspace) : nullptr;
}

int s2s_attn_beam_advance(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, int eos, int K,
                          int maxseqlength, int count, const float* logp, void* workspace, size_t workspace_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && workspace && count >= 0 && count <= maxseqlength, "beam search: bad step");
  return attn_beam_advance(static_cast<hipStream_t>(stream), to_attn(d), eos, K, maxseqlength, count, logp, workspace,
                           workspace_bytes);
}

int s2s_attn_beam_done(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, int K, int maxseqlength,
                       void* workspace, int* all_done) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && workspace && all_done, "beam search: null argument");
  return attn_beam_done(static_cast<hipStream_t>(stream), to_attn(d), K, maxseqlength, workspace, all_done);
}

int s2s_attn_beam_finish(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, int K, int maxseqlength,
                         int* out, int ldo, int* out_len, float* out_score, void* workspace) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && out && out_len && workspace, "beam search: null argument");
  return attn_beam_finish(static_cast<hipStream_t>(stream), to_attn(d), K, maxseqlength, workspace, out, ldo, out_len,
                          out_score);
}

int s2s_edit_distance(s2s_ctx* ctx, s2s_stream_t stream, int n, const int* a, const int* alen, int lda, const int* b,
                      const int* blen, int ldb, int* out) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(n == 0 || (a && alen && b && blen && out), "edit distance: null argument");
  return edit_distance(static_cast<hipStream_t>(stream), n, a, alen, lda, b, blen, ldb, out);
}

// ---------------------------------------------------------------- encoder front-ends (frontend.hip)
size_t s2s_tconv_scratch_bytes(int B, int L, int Din, int Dout, int kW) {
  return tconv_scratch_bytes(B, L, Din, Dout, kW);
}
int s2s_tconv_fwd(s2s_ctx* ctx, s2s_stream_t stream, int B, int L, int Din, int Dout, int kW, int relu, const float* x,
                  const float* W, const float* b, float* y) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(x && W && y, "TemporalConvolution: null argument");
  return tconv_fwd(static_cast<hipStream_t>(stream), B, L, Din, Dout, kW, relu, x, W, b, y);
}
int s2s_tconv_bwd(s2s_ctx* ctx, s2s_stream_t stream, int B, int L, int Din, int Dout, int kW, int relu, const float* x,
                  const float* W, const float* y, const float* dy, float* dx, int dx_accumulate, float* dW, float* db,
                  float scale, void* scratch, size_t scratch_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(x && W && dy && scratch, "TemporalConvolution: null argument");
  return tconv_bwd(static_cast<hipStream_t>(stream), B, L, Din, Dout, kW, relu, x, W, y, dy, dx, dx_accumulate, dW, db,
                   scale, scratch, scratch_bytes, ctx->wgrad_overlap ? ctx->wside : nullptr, ctx->wev);
}
int s2s_tmaxpool_fwd(s2s_ctx* ctx, s2s_stream_t stream, int B, int L, int D, int kW, int dW, const float* x, float* y,
                     int* idx) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(x && y && idx, "TemporalMaxPooling: null argument");
  return tmaxpool_fwd(static_cast<hipStream_t>(stream), B, L, D, kW, dW, x, y, idx);
}
int s2s_tmaxpool_bwd(s2s_ctx* ctx, s2s_stream_t stream, int B, int L, int D, int kW, int dW, const int* idx,
                     const float* dy, float* dx) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(idx && dy && dx, "TemporalMaxPooling: null argument");
  return tmaxpool_bwd(static_cast<hipStream_t>(stream), B, L, D, kW, dW, idx, dy, dx);
}
size_t s2s_sconv_scratch_bytes(int B, int Cin, int H, int W, int Cout, int kH, int kW) {
  return sconv_scratch_bytes(B, Cin, H, W, Cout, kH, kW);
}
int s2s_sconv_fwd(s2s_ctx* ctx, s2s_stream_t stream, int B, int Cin, int H, int W, int Cout, int kH, int kW, int relu,
                  const float* x, const float* weight, const float* bias, float* y, void* scratch,
                  size_t scratch_bytes) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(x && weight && y && scratch, "SpatialConvolutionMM: null argument");
  return sconv_fwd(static_cast<hipStream_t>(stream), B, Cin, H, W, Cout, kH, kW, relu, x, weight, bias, y, scratch,
                   scratch_bytes);
}
int s2s_sconv_bwd(s2s_ctx* ctx, s2s_stream_t stream, int B, int Cin, int H, int W, int Cout, int kH, int kW, int relu,
                  const float* x, const float* weight, const float* y, const float* dy, float* dx, int dx_accumulate,
                  float* dweight, float* dbias, float scale, void* scratch, size_t scratch_bytes, int col_from_fwd) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(x && weight && dy && scratch, "SpatialConvolutionMM: null argument");
  return sconv_bwd(static_cast<hipStream_t>(stream), B, Cin, H, W, Cout, kH, kW, relu, x, weight, y, dy, dx,
                   dx_accumulate, dweight, dbias, scale, scratch, scratch_bytes, col_from_fwd);
}
int s2s_smaxpool_fwd(s2s_ctx* ctx, s2s_stream_t stream, int B, int C, int H, int W, int kW, int kH, int dW, int dH,
                     const float* x, float* y, int* idx) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(x && y && idx, "SpatialMaxPooling: null argument");
  return smaxpool_fwd(static_cast<hipStream_t>(stream), B, C, H, W, kW, kH, dW, dH, x, y, idx);
}
int s2s_smaxpool_bwd(s2s_ctx* ctx, s2s_stream_t stream, int B, int C, int H, int W, int kW, int kH, int dW, int dH,
                     const int* idx, const float* dy, float* dx) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(idx && dy && dx, "SpatialMaxPooling: null argument");
  return smaxpool_bwd(static_cast<hipStream_t>(stream), B, C, H, W, kW, kH, dW, dH, idx, dy, dx);
}
int s2s_swap12(s2s_ctx* ctx, s2s_stream_t stream, int B, int D1, int D2, int D3, const float* x, float* y) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(x && y && x != y, "Transpose2: null or in-place argument");
  return swap12(static_cast<hipStream_t>(stream), B, D1, D2, D3, x, y);
}
int s2s_pad_batch(s2s_ctx* ctx, s2s_stream_t stream, int B, int C, int Lmax, int F, const float* src,
                  const long* offsets, const int* lengths, float* dst) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(src && offsets && lengths && dst, "pad_batch: null argument");
  return pad_batch(static_cast<hipStream_t>(stream), B, C, Lmax, F, src, offsets, lengths, dst);
}
int s2s_pad_labels(s2s_ctx* ctx, s2s_stream_t stream, int B, int Tmax, const int* src, const long* offsets,
                   const int* lengths, int* dst) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(src && offsets && lengths && dst, "pad_labels: null argument");
  return pad_labels(static_cast<hipStream_t>(stream), B, Tmax, src, offsets, lengths, dst);
}
int s2s_relu_fwd(s2s_ctx* ctx, s2s_stream_t stream, long n, const float* x, float* y) {
  S2S_TRY(set_device(ctx));
  return relu_fwd(static_cast<hipStream_t>(stream), n, x, y);
}
int s2s_relu_bwd(s2s_ctx* ctx, s2s_stream_t stream, long n, const float* x, const float* dy, float* dx) {
  S2S_TRY(set_device(ctx));
  return relu_bwd(static_cast<hipStream_t>(stream), n, x, dy, dx);
}
int s2s_logsoftmax_fwd(s2s_ctx* ctx, s2s_stream_t stream, long rows, int n, const float* x, float* y) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(x && y, "LogSoftMax: null argument");
  return logsoftmax_fwd(static_cast<hipStream_t>(stream), rows, n, x, y);
}
int s2s_logsoftmax_bwd(s2s_ctx* ctx, s2s_stream_t stream, long rows, int n, const float* y, const float* dy,
                       float* dx) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(y && dy && dx, "LogSoftMax: null argument");
  return logsoftmax_bwd(static_cast<hipStream_t>(stream), rows, n, y, dy, dx);
}

int s2s_nll_seed(s2s_ctx* ctx, s2s_stream_t stream, int B, int T, int O, const float* logp, const int* labels,
                 const int* label_lengths, int normalize, float* nll, float* dlogp) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(logp && labels && nll, "nll: null argument");
  S2S_REQUIRE(B > 0 && T > 0 && O > 0, "nll: empty dims");
  return nll_seed(static_cast<hipStream_t>(stream), B, T, O, logp, labels, normalize, nll, dlogp, label_lengths);
}

size_t s2s_optim_state_bytes(size_t n) { return optim_state_bytes(n); }

int s2s_optim_reset(s2s_ctx* ctx, s2s_stream_t stream, void* state, size_t n) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(state && n > 0, "optim: null state");
  return optim_state_reset(static_cast<hipStream_t>(stream), state, n);
}

int s2s_optim_set_noise_step(s2s_ctx* ctx, s2s_stream_t stream, void* state, size_t n, unsigned t) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(state && n > 0, "optim: null state");
  return optim_set_noise_step(static_cast<hipStream_t>(stream), state, n, t);
}

static int adadelta_step(s2s_ctx* ctx, s2s_stream_t stream, const s2s_optim_config* cfg, float* params,
                         float* grads, size_t n, void* state, const long* mats, int n_mats, float* gradnorm,
                         const float* skip_flag) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(cfg != nullptr, "optim: null config");
  S2S_REQUIRE(cfg->rho >= 0.f && cfg->rho < 1.f && cfg->eps > 0.f && cfg->maxnorm > 0.f, "optim: bad config");
  const OptimConfig c{cfg->rho,           cfg->eps,           cfg->maxnorm,       cfg->weightDecay,
                      cfg->colnorm_max,   cfg->gradnoise_eta, cfg->gradnoise_gamma, cfg->gradnoise_seed};
  // device-side guard: the update is skipped if the context's failure status (or *skip_flag) is set when it runs
  return optim_adadelta_step(static_cast<hipStream_t>(stream), c, params, grads, n, state, mats, n_mats, gradnorm,
                             ctx->status_dev, skip_flag);
}

int s2s_optim_adadelta_step(s2s_ctx* ctx, s2s_stream_t stream, const s2s_optim_config* cfg, float* params,
                            float* grads, size_t n, void* state, const long* mats, int n_mats, float* gradnorm) {
  return adadelta_step(ctx, stream, cfg, params, grads, n, state, mats, n_mats, gradnorm, nullptr);
}

int s2s_optim_adadelta_step_flag(s2s_ctx* ctx, s2s_stream_t stream, const s2s_optim_config* cfg, float* params,
                                 float* grads, size_t n, void* state, const long* mats, int n_mats, float* gradnorm,
                                 const float* skip_flag) {
  return adadelta_step(ctx, stream, cfg, params, grads, n, state, mats, n_mats, gradnorm, skip_flag);
}

int s2s_ctx_status_flag(s2s_ctx* ctx, s2s_stream_t stream, float* flag) {
  S2S_REQUIRE(ctx != nullptr && flag != nullptr, "null argument");
  S2S_CHECK_HIP(hipSetDevice(ctx->device));
  S2S_REQUIRE(ctx->status_dev != nullptr, "context has no status words");
  return status_flag(static_cast<hipStream_t>(stream), ctx->status_dev, flag);
}

// ---------------------------------------------------------------- weight noise (wnoise.hip)
// arguments are checked before the context so a bad call is named even where no context can exist
static int wnoise_config(const s2s_wnoise_config* cfg, WnoiseConfig* c) {
  S2S_REQUIRE(cfg != nullptr, "wnoise: null config");
  S2S_REQUIRE(cfg->adaptive == 0 || cfg->adaptive == 1, "wnoise: adaptive must be 0 or 1");
  S2S_REQUIRE(cfg->sigma >= 0.f && (!cfg->adaptive || cfg->sigma > 0.f), "wnoise: bad sigma");
  S2S_REQUIRE(cfg->maxnorm > 0.f && cfg->weightDecay >= 0.f && cfg->gradnoise_eta >= 0.f, "wnoise: bad config");
  S2S_REQUIRE(cfg->gradnoise_eta == 0.f || cfg->gradnoise_seed != cfg->sample_seed,
              "wnoise: sample_seed must differ from gradnoise_seed when both noises are on");
  *c = WnoiseConfig{cfg->adaptive,      cfg->lambda,          cfg->sigma,          cfg->maxnorm,    cfg->weightDecay,
                    cfg->gradnoise_eta, cfg->gradnoise_gamma, cfg->gradnoise_seed, cfg->sample_seed};
  return 0;
}

size_t s2s_wnoise_state_bytes(void) { return wnoise_state_bytes(); }

int s2s_wnoise_reset(s2s_ctx* ctx, s2s_stream_t stream, void* state) {
  S2S_REQUIRE(state != nullptr, "wnoise: null state");
  S2S_TRY(set_device(ctx));
  return wnoise_state_reset(static_cast<hipStream_t>(stream), state);
}

int s2s_wnoise_set_steps(s2s_ctx* ctx, s2s_stream_t stream, void* state, unsigned t_sample, unsigned t_gradnoise) {
  S2S_REQUIRE(state != nullptr, "wnoise: null state");
  S2S_TRY(set_device(ctx));
  return wnoise_set_steps(static_cast<hipStream_t>(stream), state, t_sample, t_gradnoise);
}

int s2s_wnoise_init(s2s_ctx* ctx, s2s_stream_t stream, const s2s_wnoise_config* cfg, const float* params,
                    float* weight, size_t n) {
  WnoiseConfig c;
  S2S_TRY(wnoise_config(cfg, &c));
  S2S_REQUIRE(params && weight && n > 0, "wnoise_init: null argument");
  S2S_TRY(set_device(ctx));
  return wnoise_init(static_cast<hipStream_t>(stream), c, params, weight, n);
}

int s2s_wnoise_sample(s2s_ctx* ctx, s2s_stream_t stream, const s2s_wnoise_config* cfg, const float* weight,
                      float* params, size_t n, void* state) {
  WnoiseConfig c;
  S2S_TRY(wnoise_config(cfg, &c));
  S2S_REQUIRE(weight && params && state && n > 0, "wnoise_sample: null argument");
  S2S_TRY(set_device(ctx));
  return wnoise_sample(static_cast<hipStream_t>(stream), c, weight, params, n, state);
}

static int wnoise_bwd(s2s_ctx* ctx, s2s_stream_t stream, const s2s_wnoise_config* cfg, const float* weight,
                      const float* params, float* grads, float* gradWeight, size_t n, const float* nll, int B,
                      void* state, float* out, const float* skip_flag) {
  WnoiseConfig c;
  S2S_TRY(wnoise_config(cfg, &c));
  S2S_REQUIRE(weight && params && grads && gradWeight && nll && state && out && n > 0,
              "wnoise_backward: null argument");
  S2S_REQUIRE(B > 0, "wnoise_backward: B must be positive");
  S2S_TRY(set_device(ctx));
  // device-side guard, as the optimizer's: skipped if the context's failure status (or *skip_flag) is set when it runs
  return wnoise_backward(static_cast<hipStream_t>(stream), c, weight, params, grads, gradWeight, n, nll, B, state,
                         out, ctx->status_dev, skip_flag);
}

int s2s_wnoise_backward(s2s_ctx* ctx, s2s_stream_t stream, const s2s_wnoise_config* cfg, const float* weight,
                        const float* params, float* grads, float* gradWeight, size_t n, const float* nll, int B,
                        void* state, float* out) {
  return wnoise_bwd(ctx, stream, cfg, weight, params, grads, gradWeight, n, nll, B, state, out, nullptr);
}

int s2s_wnoise_backward_flag(s2s_ctx* ctx, s2s_stream_t stream, const s2s_wnoise_config* cfg, const float* weight,
                             const float* params, float* grads, float* gradWeight, size_t n, const float* nll,
                             int B, void* state, float* out, const float* skip_flag) {
  return wnoise_bwd(ctx, stream, cfg, weight, params, grads, gradWeight, n, nll, B, state, out, skip_flag);
}

int s2s_wnoise_mode(s2s_ctx* ctx, s2s_stream_t stream, const s2s_wnoise_config* cfg, const float* weight,
                    float* params, size_t n) {
  WnoiseConfig c;
  S2S_TRY(wnoise_config(cfg, &c));
  S2S_REQUIRE(weight && params && n > 0, "wnoise_mode: null argument");
  S2S_TRY(set_device(ctx));
  return wnoise_mode(static_cast<hipStream_t>(stream), weight, params, n);
}

int s2s_comm_unique_id(void* out_bytes) {
  S2S_REQUIRE(out_bytes != nullptr, "null out");
  ncclUniqueId id;
  const ncclResult_t r = ncclGetUniqueId(&id);
  S2S_REQUIRE(r == ncclSuccess, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  std::memcpy(out_bytes, &id, sizeof(id));
  return 0;
}

int s2s_comm_init(s2s_ctx* ctx, const void* id_bytes, int nranks, int rank) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(id_bytes && nranks > 0 && rank >= 0 && rank < nranks, "comm: bad arguments");
  ncclUniqueId id;
  std::memcpy(&id, id_bytes, sizeof(id));
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  ctx->comm = nullptr;
  const ncclResult_t r = ncclCommInitRank(&ctx->comm, nranks, id, rank);
  S2S_REQUIRE(r == ncclSuccess, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  return 0;
}

int s2s_allreduce_sum(s2s_ctx* ctx, s2s_stream_t stream, float* buf, size_t count) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(ctx->comm != nullptr, "allreduce: s2s_comm_init first");
  const ncclResult_t r =
      ncclAllReduce(buf, buf, count, ncclFloat32, ncclSum, ctx->comm, static_cast<hipStream_t>(stream));
  S2S_REQUIRE(r == ncclSuccess, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
  return 0;
}

}  // extern "C"
