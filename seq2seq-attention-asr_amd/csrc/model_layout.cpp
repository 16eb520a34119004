// The flat parameter layout as one table (model_layout.h), and the C-ABI queries that need nothing else.
#include "model_layout.h"

#include <algorithm>

namespace s2s {

std::vector<LayerDims> enc_layers(const s2s_model_dims* d) {
  std::vector<LayerDims> v;
  int D = d->inputFrameSize;
  for (int l = 1; l <= d->numLayers; ++l) {
    const int H = l == d->numLayers ? d->outputFrameSize : d->hiddenFrameSize;
    v.push_back({D, H});
    D = 2 * H;
  }
  return v;
}

std::vector<ParamSlot> param_slots(const s2s_model_dims* d) {
  std::vector<ParamSlot> s;
  long off = 0;
  auto add = [&](long rows, long cols) {
    const long n = rows ? rows * cols : cols;
    s.push_back({off, n, rows, cols});
    off += n;
  };
  for (auto& ld : enc_layers(d))
    for (int i = 0; i < 6; ++i) add(ld.H, (long)ld.H + ld.D);
  const long A = 2L * d->outputFrameSize, Sc = d->scoreDepth, S = d->stateDepth, O = d->outputDepth,
             M = d->mlpDepth, Mk = (long)d->mlpDepth * d->maxoutWindow;
  // decoder parameters in s2s_attn order: rows x cols of the weights, {0, n} for the biases
  const long dec[S2S_ATTN_NPARAMS][2] = {{Sc, A}, {Sc, S}, {0, Sc}, {1, Sc}, {S, O}, {0, S}, {S, A}, {0, S},
                                         {S, 2 * S}, {0, S}, {S, 2 * S}, {S, 2 * S}, {S, 2 * S}, {Mk, S + A},
                                         {0, Mk}, {O, M}, {0, O}};
  for (auto& rc : dec) add(rc[0], rc[1]);
  return s;
}

const char* model_dims_error(const s2s_model_dims* d) {
  if (d == nullptr) return "null dims";
  if (!(d->B > 0 && d->L > 0 && d->T > 0)) return "model: empty B/L/T";
  if (!(d->numLayers >= 1 && d->inputFrameSize > 0)) return "model: bad encoder dims";
  if (!(d->hiddenFrameSize % 16 == 0 && d->outputFrameSize % 16 == 0))
    return "model: hidden sizes must be multiples of 16";
  return nullptr;
}

s2s_attn_dims model_attn_dims(const s2s_model_dims* d, bool lengths) {
  s2s_attn_dims a{};
  a.B = d->B; a.L = d->L; a.T = d->T;
  a.annotationDepth = 2 * d->outputFrameSize; a.scoreDepth = d->scoreDepth; a.stateDepth = d->stateDepth;
  a.outputDepth = d->outputDepth; a.mlpDepth = d->mlpDepth; a.maxoutWindow = d->maxoutWindow;
  a.penalty = d->penalty; a.dropout = d->dropout; a.dropout_seed = d->dropout_seed;
  a.dropout_mask = d->dropout_mask;
  if (lengths) {
    a.frame_lengths = d->frame_lengths;
    a.label_lengths = d->label_lengths;
  }
  return a;
}

int model_weight_matrices(const s2s_model_dims* d, long* mats) {
  if (model_dims_error(d)) return -1;
  int n = 0;
  for (const ParamSlot& p : param_slots(d)) {
    if (p.rows == 0) continue;
    if (mats) {
      const long t[3] = {p.off, p.rows, p.cols};
      std::copy(t, t + 3, mats + 3 * n);
    }
    ++n;
  }
  return n;
}

int model_bucket_count(const s2s_model_dims* d) { return model_dims_error(d) ? -1 : d->numLayers + 1; }

const char* model_bucket(const s2s_model_dims* d, int i, size_t* offset, size_t* count) {
  if (const char* e = model_dims_error(d)) return e;
  const int nl = d->numLayers;
  if (!(offset && count && i >= 0 && i <= nl)) return "bucket: bad index";
  const std::vector<ParamSlot> s = param_slots(d);
  // bucket 0: the decoder (slots 6 nl ..); bucket j >= 1: encoder layer nl - j (slots 6 l .. 6 l + 5)
  const ParamSlot &first = s[i == 0 ? dec_slot(nl, 0) : enc_slot(nl - i, 0, 0)],
                  &last = i == 0 ? s.back() : s[enc_slot(nl - i, 1, 2)];
  *offset = (size_t)first.off;
  *count = (size_t)(last.off + last.numel - first.off);
  return nullptr;
}

}  // namespace s2s

using namespace s2s;

extern "C" {

size_t s2s_model_param_count(const s2s_model_dims* d) {
  if (!d) return 0;
  const ParamSlot last = param_slots(d).back();
  return (size_t)(last.off + last.numel);
}

long s2s_model_param_offset(const s2s_model_dims* d, int i, long* numel) {
  if (!d) return -1;
  const std::vector<ParamSlot> s = param_slots(d);
  if (i < 0 || i >= (int)s.size()) return -1;
  if (numel) *numel = s[i].numel;
  return s[i].off;
}

}  // extern "C"
