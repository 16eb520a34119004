// The context behind the C ABI's opaque s2s_ctx, and what every file of the C-ABI surface shares (capi.cpp,
// model_step.cpp, capi_debug.cpp, prof.cpp).
#pragma once
#include "../../include/s2s_hip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <vector>

#include "attn.h"
#include "s2s_common.h"

struct GraphKey {
  s2s_model_dims d;
  const void* ptrs[7];
  float scale;
  int flags;
  int precision;
  void* stream;
  bool operator==(const GraphKey& o) const { return std::memcmp(this, &o, sizeof(GraphKey)) == 0; }
};

constexpr int kMaxBuckets = 17;  // decoder + up to 16 encoder layers

struct CachedGraph {
  GraphKey key;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipStream_t launched_on = nullptr;  // the stream of its last replay (drained before destroy)
  unsigned long long used = 0;        // LRU clock
};
constexpr int kGraphCacheDefault = 8;

struct s2s_ctx {
  int device = 0;
  int flags = 0;
  int precision = S2S_PREC_FP32;  // S2S_PREC_*: operand precision of the hoisted GEMMs
  hipStream_t side = nullptr;     // weight-gradient GEMMs run here beside the critical path
  hipEvent_t ev[32] = {};  // model step: 0 / 1+l wgrad forks, 13-15 prologue + join, 16-20 decoder (attn_*)
  unsigned long long* seed_dev = nullptr;  // dropout seed word read by this context's replayed graphs
  hipEvent_t bev[kMaxBuckets] = {};  // S2S_BUCKET_EVENTS: gradient bucket i is final
  // s2s_ctx_set_wgrad_overlap: the module-level backward calls fork their parameter gradients onto a stream of their
  // own (wside, event wev) -- not `side`, which the captured model steps' graphs hold
  int wgrad_overlap = 0;
  hipStream_t wside = nullptr;
  hipEvent_t wev = nullptr;
  // captured model steps, one per GraphKey (least recently used evicted past graph_cap): a caller
  // alternating shapes / buffers (a data loader's double buffers, length buckets) replays instead of
  // re-capturing every step
  std::vector<CachedGraph> graphs;
  int graph_cap = kGraphCacheDefault;
  unsigned long long graph_clock = 0;
  long captures = 0, replays = 0;
  ncclComm_t comm = nullptr;
  // failure status of the context's persistent launches (handoff.h: [0] a hand-off wait timed out, [1] a
  // launch started on an aborted region): host-coherent memory the kernels write, so every call can check
  // it without a device sync; s2s_ctx_status reads it after a stream sync and clears it
  unsigned* status_host = nullptr;
  unsigned* status_dev = nullptr;
  s2s::GemmStage lt;  // bf16 operand copies of the big bf16 GEMMs (gemm_bf16.hip), one buffer per stream
};

namespace s2s {

// every compute entry point starts here: the device, the context's GEMM precision for this call, and the
// context's failure status (capi.cpp)
int set_device(s2s_ctx* ctx);
// the stream a module-level backward issues its parameter gradients on (capi.cpp)
int wgrad_stream(s2s_ctx* ctx, hipStream_t st, hipStream_t* out);
// destroys a cached executable graph after draining the streams its replay used (model_step.cpp)
int drop_graph(s2s_ctx* ctx, CachedGraph& g);
AttnDims to_attn(const s2s_attn_dims* d);

inline bool capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return true;
  return cs != hipStreamCaptureStatusNone;
}

}  // namespace s2s
