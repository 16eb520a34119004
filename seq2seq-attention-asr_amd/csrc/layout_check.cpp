// Stand-alone host check of the flat parameter layout (model_layout.cpp), built under ASan + UBSan by
// `make layout_check`: no HIP, no GPU.  Walks the model widths of the BASELINE configs, the degenerate shapes and
// the invalid arguments, and prints the default model's table, one line per slot: index offset numel rows cols
// (tests/test_abi.py compares it with the Python layout and with the loaded library).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "model_layout.h"

using namespace s2s;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "layout_check:%d: %s\n", __LINE__, #cond);    \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

// timit/model_chorowski_baseline.lua's defaults (s2s_amd.ModelConfig()), B / L / T of BASELINE config 2
static s2s_model_dims default_dims() {
  s2s_model_dims d{};
  d.B = 32; d.L = 128; d.T = 40;
  d.inputFrameSize = 123; d.hiddenFrameSize = 256; d.outputFrameSize = 256; d.numLayers = 3;
  d.scoreDepth = 512; d.stateDepth = 256; d.outputDepth = 62; d.mlpDepth = 64; d.maxoutWindow = 7;
  return d;
}

static void check_valid(const s2s_model_dims& d) {
  CHECK(model_dims_error(&d) == nullptr);
  const int nl = d.numLayers;
  const std::vector<ParamSlot> s = param_slots(&d);
  const int n = (int)s.size();
  CHECK(n == 6 * nl + S2S_ATTN_NPARAMS);
  // slots are contiguous from 0, and the public queries read the same table
  long end = 0;
  int n2d = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(s[i].off == end && s[i].numel > 0);
    CHECK(s[i].rows == 0 ? s[i].cols == s[i].numel : s[i].rows * s[i].cols == s[i].numel);
    n2d += s[i].rows > 0;
    long numel = -1;
    CHECK(s2s_model_param_offset(&d, i, &numel) == s[i].off && numel == s[i].numel);
    CHECK(s2s_model_param_offset(&d, i, nullptr) == s[i].off);
    end += s[i].numel;
  }
  CHECK(s2s_model_param_count(&d) == (size_t)end);
  CHECK(s2s_model_param_offset(&d, -1, nullptr) == -1 && s2s_model_param_offset(&d, n, nullptr) == -1);
  for (int l = 0; l < nl; ++l) CHECK(enc_slot(l, 0, 0) == 6 * l && enc_slot(l, 1, 2) == 6 * l + 5);
  CHECK(dec_slot(nl, S2S_ATTN_NPARAMS - 1) == n - 1);
  // buckets tile the buffer exactly once: the decoder at the top, then the encoder layers top-down to offset 0
  CHECK(model_bucket_count(&d) == nl + 1);
  size_t top = (size_t)end;
  for (int i = 0; i <= nl; ++i) {
    size_t off = 0, cnt = 0;
    CHECK(model_bucket(&d, i, &off, &cnt) == nullptr);
    CHECK(cnt > 0 && off + cnt == top);
    CHECK(off == (size_t)s[i == 0 ? 6 * nl : 6 * (nl - i)].off);
    top = off;
  }
  CHECK(top == 0);
  size_t off = 0, cnt = 0;
  CHECK(model_bucket(&d, nl + 1, &off, &cnt) != nullptr && model_bucket(&d, -1, &off, &cnt) != nullptr);
  CHECK(model_bucket(&d, 0, nullptr, &cnt) != nullptr && model_bucket(&d, 0, &off, nullptr) != nullptr);
  // every weight matrix is a 2-D slot, in slot order (a buffer of exactly the reported size)
  CHECK(model_weight_matrices(&d, nullptr) == n2d);
  std::vector<long> mats(3 * (size_t)n2d);
  CHECK(model_weight_matrices(&d, mats.data()) == n2d);
  int m = 0;
  for (int i = 0; i < n; ++i) {
    if (s[i].rows == 0) continue;
    CHECK(mats[3 * m] == s[i].off && mats[3 * m + 1] == s[i].rows && mats[3 * m + 2] == s[i].cols);
    CHECK(mats[3 * m] >= s[i].off && mats[3 * m] + mats[3 * m + 1] * mats[3 * m + 2] <= s[i].off + s[i].numel);
    ++m;
  }
  CHECK(m == n2d);
  // the decoder's dims: the lengths only for the library's own step
  const int fl = 0, tl = 0;
  s2s_model_dims dl = d;
  dl.frame_lengths = &fl;
  dl.label_lengths = &tl;
  const s2s_attn_dims pub = model_attn_dims(&dl, false), own = model_attn_dims(&dl, true);
  CHECK(pub.frame_lengths == nullptr && pub.label_lengths == nullptr);
  CHECK(own.frame_lengths == &fl && own.label_lengths == &tl);
  CHECK(own.annotationDepth == 2 * d.outputFrameSize && own.scoreDepth == d.scoreDepth && own.B == d.B);
  CHECK(own.hybridAttendFeatureMaps == 0 && own.external_mlp == 0 && own.decoder_lstm == 0);
}

static void check_invalid(const s2s_model_dims* d) {
  size_t off = 0, cnt = 0;
  CHECK(model_dims_error(d) != nullptr);
  CHECK(model_weight_matrices(d, nullptr) == -1);
  CHECK(model_bucket_count(d) == -1);
  CHECK(model_bucket(d, 0, &off, &cnt) != nullptr);
}

int main() {
  const s2s_model_dims def = default_dims();
  // BASELINE configs 1-5: the widths of their models
  {
    s2s_model_dims c[5] = {def, def, def, def, def};
    c[0].B = 1;                                                                      // 1: one utterance
    c[2].B = 64; c[2].dropout = 0.5f;                                                // 3: dropout, B = 64
    c[3].L = 400; c[3].T = 200; c[3].inputFrameSize = 80; c[3].outputDepth = 29;     // 4: LibriSpeech chars
    c[4].B = 16; c[4].L = 1024; c[4].T = 200; c[4].inputFrameSize = 40; c[4].outputDepth = 29;  // 5
    for (const s2s_model_dims& d : c) check_valid(d);
  }
  // degenerate shapes
  {
    s2s_model_dims d = def;
    d.numLayers = 1; check_valid(d);
    d.numLayers = 16; check_valid(d);
    d = def; d.inputFrameSize = 1; check_valid(d);
    d = def; d.inputFrameSize = 123; check_valid(d);  // not a multiple of 32
    d = def; d.maxoutWindow = 1; check_valid(d);
    d = def; d.outputDepth = 2; check_valid(d);
    d = def; d.numLayers = 2; d.hiddenFrameSize = 128; d.outputFrameSize = 16; check_valid(d);
  }
  // invalid arguments
  {
    check_invalid(nullptr);
    CHECK(s2s_model_param_count(nullptr) == 0 && s2s_model_param_offset(nullptr, 0, nullptr) == -1);
    s2s_model_dims d = def;
    d.B = 0; check_invalid(&d);
    d = def; d.numLayers = 0; check_invalid(&d);
    CHECK(s2s_model_param_count(&d) > 0);  // the queries that check nothing stay in bounds without an encoder
    d = def; d.hiddenFrameSize = 24; check_invalid(&d);
    d = def; d.outputFrameSize = 24; check_invalid(&d);
  }
  const std::vector<ParamSlot> s = param_slots(&def);
  for (size_t i = 0; i < s.size(); ++i)
    std::printf("%zu %ld %ld %ld %ld\n", i, s[i].off, s[i].numel, s[i].rows, s[i].cols);
  return 0;
}
