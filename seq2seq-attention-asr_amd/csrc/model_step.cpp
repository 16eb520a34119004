// The model-level training step of the C ABI (encoder -> attention decoder -> NLL seed -> backward): its
// workspace layout, the order its launches are issued in, and hipGraph capture / replay of that step.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "decisions.h"
#include "gru.h"
#include "gru_persist.h"
#include "handoff.h"
#include "model_layout.h"
#include "step_knobs.h"

using namespace s2s;

namespace {

AttnDims model_attn(const s2s_model_dims* d) {
  const s2s_attn_dims a = model_attn_dims(d, true);
  return to_attn(&a);
}

int check_model_dims(const s2s_model_dims* d) {
  const char* e = model_dims_error(d);
  S2S_REQUIRE(e == nullptr, e);
  S2S_TRY(attn_check_dims(model_attn(d)));
  return 0;
}

struct ModelWs {
  std::vector<float*> saved;  // 2 per layer
  std::vector<float*> Y;      // per layer output (B, L, 2H)
  std::vector<float*> dA;     // per layer gate gradients (B, L, 6H), read by the side-stream dW GEMMs
  std::vector<float*> pack;   // per layer packed weight layouts (gru_layer_pack)
  void* attn_saved;
  void* attn_scratch;
  size_t attn_scratch_bytes;
  void* scratch;
  size_t scratch_bytes;
  float *dlogp, *nll, *logp, *dY0, *dY1;
  GemmWs gws_side;  // split-K slabs of the encoder weight-gradient GEMMs (may run on the side stream)
  float* wpart;     // the first layer's in-launch weight gradients: utterance tiles' partials (S2S_BPTT_WGRAD)
  char* gsync[2];   // the persistent GRU launches' sync regions, alternating (gru_layer_preps_next)
  float* xpad;      // (B*L, Dp) zero-padded copy of the input when inputFrameSize % 32 != 0, else null
  int Dp;
  size_t total;
};
ModelWs model_ws(const s2s_model_dims* d, void* base) {
  ModelWs w{};
  Bump bp{static_cast<char*>(base), 0, 0};
  const long B = d->B, L = d->L, T = d->T, O = d->outputDepth;
  size_t scr = 0;
  long hmax = 0;
  for (auto& ld : enc_layers(d)) {
    w.saved.push_back(bp.take<float>(B * L * 5 * ld.H));
    w.saved.push_back(bp.take<float>(B * L * 5 * ld.H));
    w.Y.push_back(bp.take<float>(B * L * 2 * ld.H));
    w.dA.push_back(bp.take<float>(B * L * 6 * ld.H));
    w.pack.push_back(bp.take<float>(gru_layer_pack_bytes(2, ld.D, ld.H) / sizeof(float)));
    size_t s = gru_layer_scratch_bytes(2, d->B, d->L, ld.D, ld.H);
    scr = s > scr ? s : scr;
    hmax = ld.H > hmax ? ld.H : hmax;
  }
  const AttnDims ad = model_attn(d);
  w.attn_saved = bp.take<char>(attn_saved_bytes(ad));
  w.attn_scratch_bytes = attn_scratch_bytes(ad);
  w.attn_scratch = bp.take<char>(w.attn_scratch_bytes);
  w.scratch = bp.take<char>(scr);
  w.scratch_bytes = scr;
  w.dlogp = bp.take<float>(B * T * O);
  w.nll = bp.take<float>(B);
  w.logp = bp.take<float>(B * T * O);
  w.dY0 = bp.take<float>(B * L * 2 * hmax);
  w.dY1 = bp.take<float>(B * L * 2 * hmax);
  w.gws_side = GemmWs{bp.take<float>(kGemmWsFloats), kGemmWsFloats};
  {
    const LayerDims l0 = enc_layers(d)[0];
    GruLayerIO io{};
    io.ndir = 2; io.B = d->B; io.L = d->L; io.D = l0.D; io.H = l0.H;
    const size_t n = gru_layer_wgrad_part_floats(io);
    w.wpart = n ? bp.take<float>(n) : nullptr;
  }
  {
    size_t sb = 0;
    for (auto& ld : enc_layers(d)) sb = std::max(sb, gru_persist_sync_bytes(d->B, d->L, ld.H));
    w.gsync[0] = bp.take<char>(sb);
    w.gsync[1] = bp.take<char>(sb);
  }
  w.Dp = (d->inputFrameSize + 31) / 32 * 32;
  w.xpad = d->inputFrameSize % 32 != 0 ? bp.take<float>(B * L * w.Dp) : nullptr;
  w.total = bp.off + 256;
  return w;
}

// fork: `side` waits for everything issued so far on `st`
int fork_to(hipStream_t st, hipStream_t side, hipEvent_t ev) {
  S2S_CHECK_HIP(hipEventRecord(ev, st));
  S2S_CHECK_HIP(hipStreamWaitEvent(side, ev, 0));
  return 0;
}

// bucket i's gradients are final on stream s (S2S_BUCKET_EVENTS); an external event node when captured
int mark_bucket(hipEvent_t* bev, int i, hipStream_t s) {
  if (!bev) return 0;
  if (!capturing(s)) {
    S2S_CHECK_HIP(hipEventRecord(bev[i], s));
    return 0;
  }
  // an event-record node appended to the capture (hipEventRecordWithFlags(..., hipEventRecordExternal)
  // is refused by this runtime): it fires on every replay, after everything captured on s so far
  hipStreamCaptureStatus cs;
  unsigned long long id = 0;
  hipGraph_t g = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  S2S_CHECK_HIP(hipStreamGetCaptureInfo_v2(s, &cs, &id, &g, &deps, &nd));
  hipGraphNode_t node;
  S2S_CHECK_HIP(hipGraphAddEventRecordNode(&node, g, deps, nd, bev[i]));
  S2S_CHECK_HIP(hipStreamUpdateCaptureDependencies(s, &node, 1, hipStreamSetCaptureDependencies));
  return 0;
}

// seed_dev: the context's dropout seed word when a captured step reads its seed from the device (the
// host writes it before each replay), else null (the seed is d->dropout_seed)
int model_step_impl(hipStream_t st, hipStream_t side, hipEvent_t* ev, hipEvent_t* bev, const s2s_model_dims* d,
                    const float* params, float* grads, const float* x, const int* labels, float scale, int flags,
                    float* logp, float* nll, void* workspace, const unsigned long long* seed_dev, unsigned* status) {
  const bool split = side != nullptr;
  ModelWs w = model_ws(d, workspace);
  const std::vector<LayerDims> layers = enc_layers(d);
  const std::vector<ParamSlot> slots = param_slots(d);
  auto P = [&](int i) -> const float* { return params + slots[i].off; };
  auto G = [&](int i) -> float* { return grads + slots[i].off; };
  const long nparams = slots.back().off + slots.back().numel;
  // gradients are first written by the side stream's weight-gradient work when split: zero them
  // there (the fork precedes every gradient writer), off the critical path
  // the step head (when fused) also writes the loss seed dlogp = -labelmask and zeroes the gradients: no side-stream
  // kernel then runs in front of it (a replayed graph ran the side branch's first two kernels -- the zeroing and the
  // seed, 15 us -- before the head)
  GruLayerIO io0{};
  io0.ndir = 2;
  io0.B = d->B;
  io0.H = layers[0].H;
  const bool head_fused = g_sync_handover && gru_layer_persistent(io0);
  // S2S_FORWARD_ONLY: encoder and decoder forward and the reported nll -- no loss seed, no backward, no gradient
  // write (grads may be null), so none of the head's fused backward pieces either
  const bool fwd_only = (flags & S2S_FORWARD_ONLY) != 0;
  const bool head_seed = head_fused && split && !fwd_only;                  // dlogp in the head
  const bool head_zero = head_seed && (flags & S2S_ZERO_GRADS);            // zeroing in the head
  // the side stream forks at the step's top (ev[13]).  Measured and rejected: forking after the head, or
  // creating the side branch's nodes after layer 1's launch (the decoder prologue then starts after layer 1 holds
  // every CU and is stretched over whole GRU layers); zeroing the gradients late on the side stream
  if (split) {
    S2S_CHECK_HIP(hipEventRecord(ev[13], st));
    S2S_CHECK_HIP(hipStreamWaitEvent(side, ev[13], 0));
  }
  if ((flags & S2S_ZERO_GRADS) && !head_zero && !fwd_only)
    S2S_TRY(zero_async(split ? side : st, grads, sizeof(float) * (size_t)nparams));
  const int B = d->B, L = d->L, T = d->T, O = d->outputDepth;
  const int nl = (int)layers.size();
  AttnDims ad = model_attn(d);
  ad.dropout_seed_dev = seed_dev;
  ad.syncs_in_prologue = g_dec_sync_prologue;  // attn_fwd_prologue runs (and is joined) before the decoder
  // the step head wrote the loss seed: the decoder forward's head launch runs the MLP head's backward too
  if (head_seed) ad.dlogp_early = w.dlogp;
  AttnParams ap;
  AttnGrads ag;
  const float** pp = reinterpret_cast<const float**>(&ap);
  float** gp = reinterpret_cast<float**>(&ag);
  for (int i = 0; i < S2S_ATTN_NPARAMS; ++i) {
    pp[i] = P(dec_slot(nl, i));
    gp[i] = grads ? G(dec_slot(nl, i)) : nullptr;
  }
  // layer-1 input padded to a multiple of 32 columns: its GEMMs then run on aligned full tiles
  const float* x0 = x;
  long ldx0 = d->inputFrameSize;
  if (w.xpad) {
    x0 = w.xpad;
    ldx0 = w.Dp;
  }
  // encoder layer l's operands (fwd: io.x is the layer input; bwd adds the grads)
  auto layer_io = [&](int l) {
    const int H = layers[l].H;
    GruLayerIO io{};
    io.ndir = 2; io.B = B; io.L = L; io.D = layers[l].D; io.H = H;
    io.x = l == 0 ? x0 : w.Y[l - 1];
    io.ldx = l == 0 ? ldx0 : 2L * layers[l - 1].H;
    io.Dx = (l == 0 && w.xpad) ? w.Dp : 0;
    for (int dd = 0; dd < 2; ++dd) {
      for (int g = 0; g < 3; ++g) io.W[dd][g] = P(enc_slot(l, dd, g));
      io.reverse[dd] = dd;
      io.y[dd] = w.Y[l] + dd * H;
      io.saved[dd] = w.saved[2 * l + dd];
    }
    io.ldy = 2L * H;
    io.packed = w.pack[l];
    io.len = d->frame_lengths;
    // the persistent launches reserve their CU while the weight-gradient GEMMs run on the side stream
    io.excl = split ? 1 : 0;
    return io;  // io.status stays null: the step harvests every sync region once, at its end
  };
  // encoder layer l's gradient operands: its dW, and with dY (B, L, 2H) the two directions' dy
  auto layer_grad = [&](int l, float* dY) {
    const int H = layers[l].H;
    GruLayerGrad gr{};
    for (int dd = 0; dd < 2; ++dd) {
      for (int g = 0; g < 3; ++g) gr.dW[dd][g] = G(enc_slot(l, dd, g));
      if (dY) gr.dy[dd] = dY + dd * H;
    }
    if (dY) gr.lddy = 2L * H;
    return gr;
  };
  // the step's head (pad, pack, the first persistent launch's sync prep) as one launch when layer 1 is persistent
  if (w.xpad && !head_fused) S2S_TRY(pad_cols_f32(st, x, d->inputFrameSize, w.xpad, B * L, d->inputFrameSize, w.Dp));
  // weight packing for every layer (both passes) and the decoder's parameter folds need only params
  // and labels: layer 1 on the critical path, the rest beside layer 1's recurrence when split
  // weight packing for every layer and both passes: one launch on the critical path (~10 us); the
  // decoder's parameter folds (params and labels only) beside the encoder when split
  // (when layer 1's persistent forward has spare slots, only what it reads is packed here; its spare slots
  // pack the rest -- the backward transposes and the later layers -- while it runs)
  GruPackJobs deferred{};
  bool defer_pack = false;
  {
    std::vector<GruLayerIO> ios;
    for (int l = 0; l < nl; ++l) ios.push_back(layer_io(l));
    defer_pack = g_defer_pack && 2 * nl <= kMaxPackJobs && gru_layer_preps_next(ios[0], true);
    if (head_fused) {
      GruStepHead extra{};
      if (head_seed) {
        extra.dlogp = w.dlogp; extra.labels = labels; extra.tlen = d->label_lengths;
        extra.B = B; extra.T = T; extra.O = O;
      }
      if (head_zero) {
        extra.zero = grads; extra.zero_n4 = (size_t)nparams / 4; extra.zero_tail = (int)(nparams % 4);
      }
      S2S_TRY(gru_step_head(st, ios.data(), w.pack.data(), nl, defer_pack ? &deferred : nullptr, x,
                            d->inputFrameSize, w.xpad, B * L, d->inputFrameSize, w.Dp, w.gsync[0],
                            gru_layer_sync_prep_bytes(ios[0]), w.gsync[1], &extra));
    }
    else
      S2S_TRY(gru_layers_pack(st, ios.data(), w.pack.data(), nl, defer_pack ? &deferred : nullptr));
    if (fwd_only && defer_pack) {  // the deferred jobs' transposes (UhT, UzrT) serve only the BPTT launches
      int n = 0;
      for (int i = 0; i < deferred.n; ++i) {
        GruPackJob job = deferred.j[i];
        job.UhT = job.UzrT = nullptr;
        if (job.Uzr || job.Uh || job.Wx) deferred.j[n++] = job;
      }
      deferred.n = n;
    }
  }
  // decoder parameter folds + dlogp = -labelmask (params and labels only): on the side stream, joined before the
  // decoder (the persistent GRU launches hold every CU, so it runs in their gaps); inline without a side stream
  if (split) {
    if (!head_seed && !fwd_only)  // dlogp = -labelmask
      S2S_TRY(nll_seed(side, B, T, O, nullptr, labels, 0, nullptr, w.dlogp, d->label_lengths));
    S2S_TRY(attn_fwd_prologue(side, ad, labels, ap, w.attn_saved, w.attn_scratch));
    S2S_CHECK_HIP(hipEventRecord(ev[14], side));
  } else {
    S2S_TRY(attn_fwd_prologue(st, ad, labels, ap, w.attn_saved, w.attn_scratch));
  }
  // the persistent GRU launches of the step (forward layers 1..nl, then backward nl..1) alternate between
  // two sync regions; a launch with spare slots prepares the next launch's region itself, so only the
  // first launch has a sync_prep in front of it
  int glaunch = 0;
  decide("step.sync_handover", g_sync_handover);
  bool gprepared = head_fused;  // the step head prepared the first launch's region
  bool gused[2] = {false, false};  // a persistent launch of this step used the region (harvested at the end)
  auto hand_over = [&](GruLayerIO& io, bool fwd, const GruLayerIO* next) {
    if (!g_sync_handover) return;
    if (gru_layer_persistent(io)) gused[glaunch & 1] = true;
    io.sync = w.gsync[glaunch & 1];
    io.sync_prepared = gprepared ? 1 : 0;
    io.sync_next = next ? w.gsync[(glaunch + 1) & 1] : nullptr;
    io.sync_next_prep = next ? gru_layer_sync_prep_bytes(*next) : 0;
    gprepared = next != nullptr && gru_layer_preps_next(io, fwd);
    ++glaunch;
  };
  // the region headers hold failure words: the first persistent launch's sync_prep clears the other region's
  // header too (sync_prep `clear`); when layer 1 runs per-step kernels, clear both here instead
  if (g_sync_handover && !gru_layer_persistent(layer_io(0))) {
    bool later = false;
    for (int l = 1; l < nl; ++l) later = later || gru_layer_persistent(layer_io(l));
    if (later)
      for (int r = 0; r < 2; ++r) S2S_TRY(zero_async(st, w.gsync[r], 256));
  }
  // ---- encoder forward (3 x BiGRU, JoinTable(2,2) by strided writes)
  for (int l = 0; l < nl; ++l) {
    GruLayerIO io = layer_io(l);
    const GruLayerIO next = layer_io(l + 1 < nl ? l + 1 : nl - 1);
    // (the last forward launch prepares the first backward launch's sync region -- when there is a backward)
    hand_over(io, true, (fwd_only && l + 1 == nl) ? nullptr : &next);
    if (l == 0 && defer_pack) io.pack_jobs = &deferred;
    S2S_TRY(gru_layer_fwd(st, io, w.scratch, w.scratch_bytes));
  }
  // ---- attention decoder forward
  if (split) S2S_CHECK_HIP(hipStreamWaitEvent(st, ev[14], 0));
  float* lp = logp ? logp : w.logp;
  S2S_TRY(attn_fwd(st, ad, w.Y[nl - 1], labels, ap, lp, w.attn_saved, w.attn_scratch, w.attn_scratch_bytes, true,
                   nullptr, nullptr));
  // ---- loss seed: dlogp = -labelmask needs only the labels (computed beside the encoder when split);
  // the reported nll (timit.lua:268-272) is computed on the side stream at the end of the step
  if (!split || fwd_only)
    S2S_TRY(nll_seed(st, B, T, O, lp, labels, (flags & S2S_NORMALIZE_NLL) ? 1 : 0, nll ? nll : w.nll,
                     fwd_only ? nullptr : w.dlogp, d->label_lengths));
  if (!fwd_only) {
    // ---- decoder backward -> dh
    float* dYcur = w.dY0;
    float* dYnext = w.dY1;
    // the decoder's dh (context term + dVh V) is produced by the top layer's BPTT launch itself when it can
    // (gru_layer_dy_fused), otherwise by GEMMs in front of it
    AttnDhTerms dht{};
    S2S_TRY(attn_bwd_core(st, ad, w.Y[nl - 1], labels, ap, w.attn_saved, w.dlogp, dYcur, 0, w.attn_scratch,
                          w.attn_scratch_bytes, nullptr, nullptr, g_fuse_dh ? &dht : nullptr));
    // the decoder's weight gradients beside the top BPTT (side stream).  (Creating their nodes after the top BPTT's
    // launch measured 3.167 -> 3.680 ms: the replayed graph then ran the whole side branch after the last BPTT.)
    if (split) {
      S2S_CHECK_HIP(hipEventRecord(ev[0], st));
      S2S_CHECK_HIP(hipStreamWaitEvent(side, ev[0], 0));
    }
    S2S_TRY(attn_bwd_wgrad(split ? side : st, ad, w.Y[nl - 1], labels, ap, w.attn_saved, ag, scale, w.attn_scratch));
    S2S_TRY(mark_bucket(bev, 0, split ? side : st));
    // the reported nll (timit.lua:268-272) beside the encoder BPTT
    if (split)
      S2S_TRY(nll_seed(side, B, T, O, lp, labels, (flags & S2S_NORMALIZE_NLL) ? 1 : 0, nll ? nll : w.nll, nullptr,
                       d->label_lengths));
    // ---- encoder backward.  Layer l's weight-gradient GEMMs (side stream) wait for an event recorded between layer
    // l-1's BPTT sync prep and its launch, so the persistent BPTT is dispatched before the GEMM's workgroups take the
    // CUs (forked right after layer l's own BPTT, the replayed graph started the GEMM first and layers 2 and 1's BPTT
    // ran 590-618 us instead of 533-540 us, profiles/r01)
    const bool defer = split;
    int pending = -1;  // layer whose weight gradients wait for the next BPTT's sync prep
    auto issue_wgrad = [&](int l) -> int {
      const GruLayerIO io = layer_io(l);
      GruLayerGrad gr = layer_grad(l, nullptr);
      gr.scale = scale;
      S2S_TRY(gru_layer_wgrad(split ? side : st, io, gr, w.dA[l], w.gws_side));
      S2S_TRY(mark_bucket(bev, nl - l, split ? side : st));
      return 0;
    };
    for (int l = nl - 1; l >= 0; --l) {
      const int H = layers[l].H;
      GruLayerIO io = layer_io(l);
      const GruLayerIO next = layer_io(l > 0 ? l - 1 : 0);
      hand_over(io, false, l > 0 ? &next : nullptr);
      GruLayerGrad gr = layer_grad(l, dYcur);
      // this layer's dX is the dy of the layer below: produced inside that layer's BPTT launch (or by one
      // GEMM in front of it), so the critical path has no GEMM between two BPTT launches
      gr.dx = nullptr;
      if (l == nl - 1 && dht.dvh) {  // dy = dh = sum_t alpha dc + dVh V, in-launch
        gr.ydA = dht.dvh;
        gr.yldA = dht.Sc;
        gr.yK = dht.Sc;
        gr.yN = dht.A;
        gr.yWx = dht.V;
        gr.yldw = dht.A;
        gr.yalpha = dht.alpha;
        gr.ydc = dht.dc;
        gr.yT = dht.T;
        if (dht.A != 2 * H || !gru_layer_dy_fused(io, gr)) {
          gr = layer_grad(l, dYcur);
          S2S_TRY(attn_dh_gemms(st, dht, dYcur, 0));
        }
      }
      if (l + 1 < nl) {
        const GruLayerIO up = layer_io(l + 1);
        gr.ydA = w.dA[l + 1];
        gr.yldA = 3L * up.ndir * up.H;
        gr.yK = 3 * up.ndir * up.H;
        gr.yN = up.D;
        gr.yWx = gru_layer_packed_wx(up, &gr.yldw);
        S2S_REQUIRE(gr.yWx != nullptr && up.ldx == 2L * H, "model step: dX of layer above needs packed weights");
      }
      gr.scale = scale;
      // the first layer's weight gradients inside its BPTT launch: nothing behind the step's last recurrence
      const bool wg_in = l == 0 && g_bptt_wgrad && gru_layer_wgrad_fused(io);
      if (wg_in) {
        gr.wgrad = 1;
        gr.wpart = w.wpart;
      }
      if (l == 0) decide("step.bptt_wgrad_in", wg_in);
      if (l == nl - 1) decide("step.fuse_dh", gr.yalpha != nullptr);  // the decoder's dh inside the top BPTT launch
      if (defer && pending >= 0) gr.prep_event = ev[1 + pending];
      S2S_TRY(gru_layer_bwd_core(st, io, gr, w.dA[l], w.scratch, w.scratch_bytes));
      if (defer) {
        if (pending >= 0) {  // the layer above: after this BPTT's dispatch point
          S2S_CHECK_HIP(hipStreamWaitEvent(side, ev[1 + pending], 0));
          S2S_TRY(issue_wgrad(pending));
        }
        pending = l;
        if (l == 0 && wg_in) {
          S2S_TRY(mark_bucket(bev, nl, st));
        } else if (l == 0) {  // the last BPTT: nothing left to dispatch ahead of layer 1's GEMMs
          S2S_TRY(fork_to(st, side, ev[1 + l]));
          S2S_TRY(issue_wgrad(l));
        }
      } else if (wg_in) {
        S2S_TRY(mark_bucket(bev, nl - l, st));
      } else {
        if (split) S2S_TRY(fork_to(st, side, ev[1 + l]));
        S2S_TRY(gru_layer_wgrad(split ? side : st, io, gr, w.dA[l], w.gws_side));
        S2S_TRY(mark_bucket(bev, nl - l, split ? side : st));
      }
      float* tmp = dYcur;
      dYcur = dYnext;
      dYnext = tmp;
    }
  }
  // failure words of every sync region the step's persistent launches used -> the context's status (handoff.h),
  // on the main stream after the last BPTT (beside the side stream's weight-gradient tail)
  if (status) {
    void* regions[4];
    int nr = 0;
    for (int r = 0; r < 2; ++r)
      if (gused[r]) regions[nr++] = w.gsync[r];
    nr += attn_sync_regions(ad, w.attn_saved, w.attn_scratch, &regions[nr], &regions[nr + 1]);
    S2S_TRY(launch_sync_harvest(st, regions, nr, status));
  }
  if (split) {  // join: the step ends when the side stream's gradient GEMMs are done
    S2S_CHECK_HIP(hipEventRecord(ev[15], side));
    S2S_CHECK_HIP(hipStreamWaitEvent(st, ev[15], 0));
  }
  return 0;
}

// drops the least recently used cached graph
int evict_lru(s2s_ctx* ctx) {
  size_t lru = 0;
  for (size_t i = 1; i < ctx->graphs.size(); ++i)
    if (ctx->graphs[i].used < ctx->graphs[lru].used) lru = i;
  S2S_TRY(drop_graph(ctx, ctx->graphs[lru]));
  ctx->graphs.erase(ctx->graphs.begin() + (long)lru);
  return 0;
}

}  // namespace

// Destroy a cached executable graph.  A replay of it may still be running (the host runs ahead of the
// device): HIP's hipGraphExecDestroy frees the executable's kernel-argument and node storage at once
// instead of deferring the free to the end of an in-flight launch (CUDA's documented behaviour), so
// destroying it under a running replay is a use-after-free in the runtime -- the round-1 segfaults
// inside s2s_model_step, which re-captured (and destroyed the previous exec) on every dropout step.
// Drain the streams the replay used first.
int s2s::drop_graph(s2s_ctx* ctx, CachedGraph& g) {
  if (g.exec) {
    if (g.launched_on) S2S_CHECK_HIP(hipStreamSynchronize(g.launched_on));
    if (ctx->side) S2S_CHECK_HIP(hipStreamSynchronize(ctx->side));
    (void)hipGraphExecDestroy(g.exec);
  }
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr;
  g.graph = nullptr;
  return 0;
}

extern "C" {

size_t s2s_model_workspace_bytes(const s2s_model_dims* d) {
  if (check_model_dims(d) != 0) return 0;
  return model_ws(d, nullptr).total;
}

int s2s_model_attn_dims(const s2s_model_dims* d, s2s_attn_dims* out) {
  S2S_REQUIRE(d != nullptr && out != nullptr, "null argument");
  *out = model_attn_dims(d, false);
  return 0;
}

const void* s2s_model_attn_saved(const s2s_model_dims* d, const void* workspace) {
  if (!d || !workspace || check_model_dims(d) != 0) return nullptr;
  ModelWs w = model_ws(d, const_cast<void*>(workspace));
  return w.attn_saved;
}

const float* s2s_model_encoder_output(const s2s_model_dims* d, const void* workspace) {
  if (!d || !workspace) return nullptr;
  ModelWs w = model_ws(d, const_cast<void*>(workspace));
  return w.Y.back();
}

int s2s_model_weight_matrices(const s2s_model_dims* d, long* mats) {
  if (check_model_dims(d) != 0) return -1;
  return model_weight_matrices(d, mats);
}

int s2s_model_bucket_count(const s2s_model_dims* d) {
  if (check_model_dims(d) != 0) return -1;
  return model_bucket_count(d);
}

int s2s_model_bucket(const s2s_model_dims* d, int i, size_t* offset, size_t* count) {
  S2S_TRY(check_model_dims(d));
  const char* e = model_bucket(d, i, offset, count);
  S2S_REQUIRE(e == nullptr, e);
  return 0;
}

int s2s_model_step(s2s_ctx* ctx, s2s_stream_t stream, const s2s_model_dims* d, const float* params, float* grads,
                   const float* x, const int* labels, float scale, int flags, float* logp, float* nll,
                   void* workspace, size_t workspace_bytes) {
  S2S_TRY(set_device(ctx));
  // the model step keeps its GEMMs on gemm_f32's tiles: it is captured into a HIP graph at its first call (graph
  // mode), where the big GEMM's staging buffer could not be grown
  set_gemm_stage(nullptr);
  S2S_TRY(check_model_dims(d));
  S2S_REQUIRE(params && x && labels && workspace, "model: null argument");
  S2S_REQUIRE(grads || (flags & S2S_FORWARD_ONLY), "model: null gradients (only S2S_FORWARD_ONLY runs without)");
  S2S_REQUIRE(!(flags & S2S_FORWARD_ONLY) || !(flags & S2S_BUCKET_EVENTS),
              "model: S2S_FORWARD_ONLY with S2S_BUCKET_EVENTS (a forward-only step finishes no gradient bucket)");
  S2S_REQUIRE(workspace_bytes >= model_ws(d, nullptr).total, "model: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipEvent_t* bev = nullptr;
  if (flags & S2S_BUCKET_EVENTS) {
    S2S_REQUIRE(d->numLayers + 1 <= kMaxBuckets, "model: too many layers for S2S_BUCKET_EVENTS");
    for (auto& e : ctx->bev)
      if (!e) S2S_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    bev = ctx->bev;
  }
  if (!(ctx->flags & S2S_CTX_GRAPH) || st == nullptr)
    return model_step_impl(st, (st && (ctx->flags & S2S_CTX_OVERLAP)) ? ctx->side : nullptr, ctx->ev, bev, d,
                           params, grads, x, labels, scale, flags, logp, nll, workspace, nullptr, ctx->status_dev);
  // In-kernel dropout draws from a new seed every step: the replayed graph reads it from the context's
  // device word, written before each replay, so the seed is not part of the graph key.  Injected masks
  // (or no dropout) leave the seed unread: it is not part of the key either.
  const bool dev_seed = d->dropout > 0.f && d->dropout_mask == nullptr;
  if (dev_seed && !ctx->seed_dev) S2S_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->seed_dev), 64));
  GraphKey key;
  std::memset(&key, 0, sizeof(key));
  key.d = *d;
  key.d.dropout_seed = 0;
  const void* ptrs[7] = {params, grads, x, labels, logp, nll, workspace};
  std::memcpy(key.ptrs, ptrs, sizeof(ptrs));
  key.scale = scale;
  key.flags = flags;
  key.precision = ctx->precision;
  key.stream = stream;
  CachedGraph* hit = nullptr;
  for (auto& g : ctx->graphs)
    if (g.key == key) hit = &g;
  if (!hit) {
    if ((int)ctx->graphs.size() >= ctx->graph_cap) S2S_TRY(evict_lru(ctx));
    S2S_CHECK_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = model_step_impl(st, (ctx->flags & S2S_CTX_OVERLAP) ? ctx->side : nullptr, ctx->ev, bev, d,
                                   params, grads, x, labels, scale, flags, logp, nll, workspace,
                                   dev_seed ? ctx->seed_dev : nullptr, ctx->status_dev);
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(st, &g);
    if (rc != 0) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    S2S_CHECK_HIP(ec);
    CachedGraph cg;
    cg.key = key;
    cg.graph = g;
    const hipError_t ei = hipGraphInstantiate(&cg.exec, g, nullptr, nullptr, 0);
    if (ei != hipSuccess) {
      (void)hipGraphDestroy(g);
      S2S_CHECK_HIP(ei);
    }
    ctx->graphs.push_back(cg);
    hit = &ctx->graphs.back();
    ctx->captures += 1;
  }
  hit->used = ++ctx->graph_clock;
  hit->launched_on = st;
  if (dev_seed) S2S_TRY(set_device_u64(st, ctx->seed_dev, d->dropout_seed));
  S2S_CHECK_HIP(hipGraphLaunch(hit->exec, st));
  ctx->replays += 1;
  return 0;
}

int s2s_ctx_graph_stats(s2s_ctx* ctx, long* captures, long* replays, int* cached) {
  S2S_REQUIRE(ctx != nullptr, "null context");
  if (captures) *captures = ctx->captures;
  if (replays) *replays = ctx->replays;
  if (cached) *cached = (int)ctx->graphs.size();
  return 0;
}

int s2s_ctx_set_graph_cache(s2s_ctx* ctx, int capacity) {
  S2S_REQUIRE(ctx != nullptr, "null context");
  S2S_REQUIRE(capacity >= 1 && capacity <= 64, "graph cache capacity must be in [1, 64]");
  S2S_TRY(set_device(ctx));
  ctx->graph_cap = capacity;
  while ((int)ctx->graphs.size() > capacity) S2S_TRY(evict_lru(ctx));
  return 0;
}

int s2s_stream_wait_bucket(s2s_ctx* ctx, s2s_stream_t stream, int i) {
  S2S_TRY(set_device(ctx));
  S2S_REQUIRE(i >= 0 && i < kMaxBuckets && ctx->bev[i], "bucket: no event (step without S2S_BUCKET_EVENTS?)");
  S2S_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), ctx->bev[i], 0));
  return 0;
}

}  // extern "C"
