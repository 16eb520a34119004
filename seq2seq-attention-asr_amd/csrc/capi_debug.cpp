// The s2s_debug_* entry points of the C-ABI layer: diagnostics, test probes and A/B knobs exported by libs2s_hip.so
// but not part of the C ABI header (include/s2s_hip.h).  (The kernels' own knobs sit beside their kernels.)
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "ctx.h"
#include "decisions.h"
#include "gru_persist.h"
#include "step_knobs.h"

using namespace s2s;

// diagnostic: one GEMM C = alpha op(A) op(B) + beta C through the library's MFMA GEMM (bf16 = 1: the bf16-operand
// kernels), on the legacy default stream; for the layout tests
extern "C" int s2s_debug_gemm(int transA, int transB, int M, int N, int K, float alpha, const float* A, long lda,
                              const float* B, long ldb, float beta, float* C, long ldc, int bf16, float* ws,
                              size_t ws_floats) {
  s2s::set_gemm_precision(bf16 ? s2s::kGemmBf16 : s2s::kGemmF32);
  const int rc = s2s::gemm1(nullptr, transA != 0, transB != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, nullptr,
                            s2s::GemmWs{ws, ws ? ws_floats : 0});
  s2s::set_gemm_precision(s2s::kGemmF32);
  return rc;
}
// test entries (tests/test_gpu_gemm_f32.py): a batch of problems straight on the fp32 MFMA GEMM, and the plan that
// call launched (s2s::gemm_last_plan: filled by gemm_f32 itself, not recomputed here)
struct s2s_debug_gemm_problem {  // s2s::GemmProblem as plain C
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* rbias;
  long lda, ldb, ldc;
  int M, N, K;
  float alpha, beta;
  int Mread, Nread, relu;
};
struct s2s_debug_gemm_plan {
  int launched, bm, bn, kslice, nblocks, reduced;
  int splits[s2s::kMaxGemmBatch];  // per problem, in the caller's order; 0 = skipped
};
static s2s::GemmProblem to_problem(const s2s_debug_gemm_problem& q) {
  s2s::GemmProblem p{q.A, q.B, q.C, q.bias, q.lda, q.ldb, q.ldc, q.M, q.N, q.K, q.alpha, q.beta};
  p.Mread = q.Mread;
  p.Nread = q.Nread;
  p.rbias = q.rbias;
  p.relu = q.relu;
  return p;
}
// the same with the operand precision (tests/test_gpu_gemm_bf16.py): bf16 = 1 runs gemm_f32's bf16 tile family
// (gemm_bf16_kernel) on every problem -- it clears the calling thread's staging buffer (every C-ABI entry with a
// context sets it again), so none goes to the big-tile GEMM
extern "C" int s2s_debug_gemm_batch_prec(s2s_stream_t stream, const s2s_debug_gemm_problem* probs, int nprob, int transA,
                                         int transB, int bf16, float* ws, size_t ws_floats, s2s_debug_gemm_plan* plan) {
  S2S_REQUIRE(probs != nullptr && plan != nullptr, "debug_gemm_batch: null argument");
  S2S_REQUIRE(nprob >= 1 && nprob <= s2s::kMaxGemmBatch,
              "debug_gemm_batch: 1 .. " + std::to_string(s2s::kMaxGemmBatch) + " problems");
  s2s::GemmProblem p[s2s::kMaxGemmBatch];
  for (int i = 0; i < nprob; ++i) p[i] = to_problem(probs[i]);
  if (bf16) s2s::set_gemm_stage(nullptr);
  s2s::set_gemm_precision(bf16 ? s2s::kGemmBf16 : s2s::kGemmF32);
  const int rc = s2s::gemm_f32(static_cast<hipStream_t>(stream), p, nprob, transA != 0, transB != 0,
                               s2s::GemmWs{ws, ws ? ws_floats : 0});
  s2s::set_gemm_precision(s2s::kGemmF32);
  const s2s::GemmLastPlan& lp = s2s::gemm_last_plan();
  *plan = s2s_debug_gemm_plan{lp.launched, lp.bm, lp.bn, lp.kslice, lp.nblocks, lp.reduced, {}};
  for (int i = 0; i < s2s::kMaxGemmBatch; ++i) plan->splits[i] = lp.splits[i];
  return rc;
}
extern "C" int s2s_debug_gemm_batch(s2s_stream_t stream, const s2s_debug_gemm_problem* probs, int nprob, int transA,
                                    int transB, float* ws, size_t ws_floats, s2s_debug_gemm_plan* plan) {
  return s2s_debug_gemm_batch_prec(stream, probs, nprob, transA, transB, 0, ws, ws_floats, plan);
}
// one thin entry per helper of gemm_f32.hip
extern "C" int s2s_debug_colsum(s2s_stream_t stream, const float* X, long ldx, int M, int N, float alpha, float beta,
                                float* out, float* ws, size_t ws_floats) {
  return s2s::colsum_f32(static_cast<hipStream_t>(stream), X, ldx, M, N, alpha, beta, out,
                         s2s::GemmWs{ws, ws ? ws_floats : 0});
}
struct s2s_debug_colsum_out {  // s2s::ColsumOut
  int col0, ncols;
  float* dst[3];
  int ndst;
};
extern "C" int s2s_debug_colsum_scatter(s2s_stream_t stream, const float* X, long ldx, int M, int N, float alpha,
                                        const s2s_debug_colsum_out* outs, int nouts, float* ws, size_t ws_floats) {
  S2S_REQUIRE(nouts >= 0 && nouts <= s2s::kMaxColsumOuts,
              "debug_colsum_scatter: at most " + std::to_string(s2s::kMaxColsumOuts) + " output ranges");
  S2S_REQUIRE(outs != nullptr || nouts == 0, "debug_colsum_scatter: null argument");
  s2s::ColsumOut o[s2s::kMaxColsumOuts];
  for (int e = 0; e < nouts; ++e)
    o[e] = s2s::ColsumOut{outs[e].col0, outs[e].ncols, {outs[e].dst[0], outs[e].dst[1], outs[e].dst[2]}, outs[e].ndst};
  return s2s::colsum_scatter_f32(static_cast<hipStream_t>(stream), X, ldx, M, N, alpha, o, nouts,
                                 s2s::GemmWs{ws, ws ? ws_floats : 0});
}
extern "C" int s2s_debug_copy2d(s2s_stream_t stream, const float* src, long lds, float* dst, long ldd, int rows,
                                int cols, int accumulate) {
  return s2s::copy2d_f32(static_cast<hipStream_t>(stream), src, lds, dst, ldd, rows, cols, accumulate != 0);
}
extern "C" int s2s_debug_transpose(s2s_stream_t stream, const float* src, long lds, int rows, int cols, float* dst,
                                   long ldd) {
  return s2s::transpose_f32(static_cast<hipStream_t>(stream), src, lds, rows, cols, dst, ldd);
}
extern "C" int s2s_debug_pad_cols(s2s_stream_t stream, const float* src, long lds, float* dst, int rows, int cols,
                                  int dcols) {
  return s2s::pad_cols_f32(static_cast<hipStream_t>(stream), src, lds, dst, rows, cols, dcols);
}
extern "C" int s2s_debug_axpby(s2s_stream_t stream, const float* src, float* dst, size_t n, float alpha, float beta) {
  return s2s::axpby_f32(static_cast<hipStream_t>(stream), src, dst, n, alpha, beta);
}
extern "C" int s2s_debug_fill_u32(s2s_stream_t stream, void* dst, unsigned value, size_t count) {
  return s2s::fill_u32_async(static_cast<hipStream_t>(stream), dst, value, count);
}
extern "C" int s2s_debug_zero(s2s_stream_t stream, void* dst, size_t bytes) {
  return s2s::zero_async(static_cast<hipStream_t>(stream), dst, bytes);
}
// test / bench entry: one problem straight on the big-tile bf16 GEMM (gemm_bf16.hip) with the context's staging
// buffer; *done = 0 when the kernel declined it (nothing launched)
extern "C" int s2s_debug_gemm_big_run(s2s_ctx* ctx, s2s_stream_t stream, int transA, int transB, int M, int N, int K,
                                      float alpha, const float* A, long lda, const float* B, long ldb, float beta,
                                      float* C, long ldc, const float* bias, int relu, int* done) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(done != nullptr, "null argument");
  s2s::GemmProblem q{A, B, C, bias, lda, ldb, ldc, M, N, K, alpha, beta};
  q.relu = relu;
  bool d = false;
  const int rc = s2s::gemm_big_bf16(static_cast<hipStream_t>(stream), q, transA != 0, transB != 0, &d);
  *done = d ? 1 : 0;
  return rc;
}
// the same from a whole problem description (rbias, Mread, Nread: what the big-tile GEMM must decline)
extern "C" int s2s_debug_gemm_big_problem(s2s_ctx* ctx, s2s_stream_t stream, const s2s_debug_gemm_problem* prob,
                                          int transA, int transB, int* done) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(prob != nullptr && done != nullptr, "null argument");
  bool d = false;
  const int rc = s2s::gemm_big_bf16(static_cast<hipStream_t>(stream), to_problem(*prob), transA != 0, transB != 0, &d);
  *done = d ? 1 : 0;
  return rc;
}
// diagnostic: every finished hypothesis of a beam search still in its workspace (the reference's y_finished /
// p_finished, Attention.lua:375-376): nfin (B), flen (B*K), fscore (B*K), fseq (B*K*(maxseqlength+1)) device
// buffers, filled in stream order; entries at or beyond nfin[b] are unspecified (tests/test_gpu_decode.py)
extern "C" int s2s_debug_beam_finished(s2s_ctx* ctx, s2s_stream_t stream, const s2s_attn_dims* d, int K,
                                       int maxseqlength, void* workspace, int* nfin, int* flen, float* fscore,
                                       int* fseq) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(d && workspace && nfin && flen && fscore && fseq, "beam search: null argument");
  return attn_beam_finished(static_cast<hipStream_t>(stream), to_attn(d), K, maxseqlength, workspace, nfin, flen,
                            fscore, fseq);
}
// diagnostic: the context's 16 status words ([0] timeout, [1] aborted region, [4 + i] raw failure bits of the
// last harvest's region i) -- tools/status_diag.py
extern "C" int s2s_debug_status_words(s2s_ctx* ctx, unsigned* out16) {
  S2S_REQUIRE(ctx && out16, "null argument");
  for (int i = 0; i < 16; ++i) out16[i] = ctx->status_host ? __atomic_load_n(ctx->status_host + i, __ATOMIC_ACQUIRE) : 0u;
  return 0;
}
// test probe: one wave of a persistent-style launch that waits for a value nobody writes (region: >= 768 bytes
// of device memory); the context's status must then read S2S_STATUS_HANDOFF_TIMEOUT
extern "C" int s2s_debug_handoff_timeout(s2s_ctx* ctx, s2s_stream_t stream, void* region) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(region != nullptr, "null region");
  return handoff_timeout_probe_launch(static_cast<hipStream_t>(stream), region, ctx->status_dev);
}
// test knob: the next n sync_preps (any context) start their region aborted, so the persistent launch behind
// each reports S2S_STATUS_ABORTED_REGION and returns at once (tests/test_gpu_status.py)
static std::atomic<int> g_inject_abort{0};
extern "C" void s2s_debug_inject_abort(int n) { g_inject_abort = n; }
int s2s::inject_abort_take() {
  int v = g_inject_abort.load(std::memory_order_relaxed);
  while (v > 0 && !g_inject_abort.compare_exchange_weak(v, v - 1)) {
  }
  return v > 0 ? 1 : 0;
}
// the record of dispatch decisions (decisions.h): name -> (last value, count), filled by the code that decides
static std::mutex g_decisions_mu;
static std::map<std::string, std::pair<long, long>> g_decisions;
std::atomic<int> s2s::g_decisions_on{0};
void s2s::decision_store(const char* name, long value) {
  std::lock_guard<std::mutex> lock(g_decisions_mu);
  std::pair<long, long>& e = g_decisions[name];
  e.first = value;
  e.second += 1;
}
extern "C" void s2s_debug_decisions(int on) { s2s::g_decisions_on.store(on ? 1 : 0, std::memory_order_relaxed); }
extern "C" void s2s_debug_decisions_clear() {
  std::lock_guard<std::mutex> lock(g_decisions_mu);
  g_decisions.clear();
}
// 1 and *value / *count when `name` was recorded since the last clear, else 0 (and both 0)
extern "C" int s2s_debug_decision(const char* name, long* value, long* count) {
  std::lock_guard<std::mutex> lock(g_decisions_mu);
  const auto it = name ? g_decisions.find(name) : g_decisions.end();
  const bool have = it != g_decisions.end();
  if (value) *value = have ? it->second.first : 0;
  if (count) *count = have ? it->second.second : 0;
  return have ? 1 : 0;
}
// the model step's knobs (step_knobs.h)
extern "C" void s2s_debug_fuse_dh(int on) { g_fuse_dh = on; }
extern "C" void s2s_debug_sync_handover(int on) { g_sync_handover = on; }
extern "C" void s2s_debug_dec_sync_prologue(int on) { g_dec_sync_prologue = on; }
extern "C" void s2s_debug_defer_pack(int on) { g_defer_pack = on; }
extern "C" void s2s_debug_bptt_wgrad(int on) { g_bptt_wgrad = on; }
