// Process-wide diagnostic knobs of the model step (s2s_debug_*, capi_debug.cpp; not in the C ABI header; A/B tools
// and tests only), read when model_step.cpp issues its launches; no per-step state lives in globals (exclusive-CU
// mode, precision and the failure status are per call / per context)
#pragma once
#include <atomic>

namespace s2s {

// s2s_debug_bptt_wgrad(1) (A/B, tests): the first encoder layer's weight gradients inside its BPTT launch
// (gru_persist.hip bptt_wgrad) instead of a GEMM behind it on the side stream (measured slower)
inline std::atomic<int> g_bptt_wgrad{0};
inline std::atomic<int> g_defer_pack{1};  // s2s_debug_defer_pack(0): every layer packed in front of layer 1
inline std::atomic<int> g_dec_sync_prologue{1};  // s2s_debug_dec_sync_prologue(0): decoder sync preps in place
inline std::atomic<int> g_sync_handover{1};  // s2s_debug_sync_handover(0): a sync_prep in front of every GRU launch
inline std::atomic<int> g_fuse_dh{1};  // s2s_debug_fuse_dh(0): the decoder's dh by GEMMs in front of the top BPTT

}  // namespace s2s
