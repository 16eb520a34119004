// The model's flat parameter layout (include/s2s_hip.h "whole training step"): what every
// trainer, optimizer, all-reduce bucket and checkpoint indexes the parameter and gradient buffers by.
// Host-only arithmetic: this header and model_layout.cpp include no HIP, so layout_check.cpp compiles
// them with a plain host compiler under sanitizers (make layout_check).
#pragma once
#include <vector>

#include "../../include/s2s_hip.h"

namespace s2s {

struct LayerDims {
  int D, H;
};
// input and hidden width of every encoder layer (the last one's hidden width is outputFrameSize)
std::vector<LayerDims> enc_layers(const s2s_model_dims* d);

// One parameter of the flat buffer: offset and element count in floats; rows x cols of a weight
// (W = (out, in)), rows == 0 for a 1-D parameter (cols = numel).  Order: encoder layers x (fwd, bwd)
// x (Wz, Wr, Wh), then the decoder in s2s_attn order.
struct ParamSlot {
  long off, numel, rows, cols;
};
std::vector<ParamSlot> param_slots(const s2s_model_dims* d);
inline int enc_slot(int l, int dir, int gate) { return 6 * l + 3 * dir + gate; }
inline int dec_slot(int num_layers, int i) { return 6 * num_layers + i; }

// the host-only half of the model dims check: null for dims it accepts, else the message (the library's
// check_model_dims adds the decoder's attn_check_dims)
const char* model_dims_error(const s2s_model_dims* d);
// the model's decoder as s2s_attn_dims; the frame / label lengths are carried only when `lengths`
s2s_attn_dims model_attn_dims(const s2s_model_dims* d, bool lengths);

// s2s_model_weight_matrices / s2s_model_bucket_count / s2s_model_bucket for dims whose decoder the caller has
// checked: -1 for dims model_dims_error rejects; model_bucket returns null or the message of its failure
int model_weight_matrices(const s2s_model_dims* d, long* mats);
int model_bucket_count(const s2s_model_dims* d);
const char* model_bucket(const s2s_model_dims* d, int i, size_t* offset, size_t* count);

}  // namespace s2s
