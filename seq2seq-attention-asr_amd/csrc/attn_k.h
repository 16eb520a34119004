// The attention decoder's kernel arguments, workspace layout and route: shared by attn.hip and the files it includes
// (attn_layout.inc, dec_steps.inc, attn_persist.inc, dec_xcd.inc, dec_xcd_lstm.inc, beam.inc), one translation unit.
#pragma once
#include "attn.h"
#include "handoff.h"
namespace s2s {
namespace {
constexpr int LC = 16;  // frames per attention workgroup (4 waves x 4 frames)

struct AttnK {
  // dims
  int B, L, T, A, Sc, S, O, M, K, NCH, t;
  float penalty;
  int hk, hf;  // hybrid attention filter size / feature maps (hf = 0: off)
  const int *flen, *tlen;  // variable-length batch: frames / labels per utterance (null: L / T)
  // params
  AttnParams P;
  const float* h;
  const int* labels;
  // saved
  float *Vh, *WS, *E, *ALPHA, *LSE, *IND, *C, *HX, *RHX, *CY, *GSV, *VV, *MM, *LOGP, *MASK;
  int* AM;
  // fwd scratch
  float *PM, *PL, *PC, *U;
  // the MLP GEMM's unreduced split-K slabs (UPS > 1: U = sum of UP[s * UPMN + e] in slice order + bm, summed by the
  // MLP head instead of a reduce launch in front of it), or null
  const float* UP;
  int UPS;
  long UPMN;
  // bwd scratch
  float *DO, *DU, *DV, *DGA, *DS, *DSP, *DSPF, *DD, *DCY, *DC, *DVH, *PDWS, *DWS, *DWEACC, *YP;
  // hybrid attention: HGT (kW, Sc) = (U W)^T and HCU (Sc) = U b (saved); QA [2][B][L][kW] the
  // d alpha_{t-1} partials q_{l,i} of the step after; PDG [B*NCH][kW][Sc] dG partials; DGT, DCU (bwd)
  float *HGT, *HCU, *QA, *PDG, *DGT, *DCU;
  float *WhT, *GT, *WdT, *WcT, *WsT;
  // decoder LSTM: LW (4S, 2S) rows [Wqh | Wqx] per gate q in (i, f, g, o), LB (4S) = bqx + bqh (saved),
  // LC (B*T, S) cell states (saved), LDW (4S, 2S) weight-gradient staging (bwd scratch); GT holds LW^T
  float *LW, *LB, *LC, *LDW;
  int lstm;
  // persistent-kernel granule buffers ([2 slots][...]) and abort word; one zeroed region each
  granule_t *gS, *gWS, *gPM, *gPL, *gPC, *gC, *gCY, *gD, *gQ;           // forward
  granule_t *gZ, *gR, *gH, *gDD, *gDCY, *gDC, *gPDWS, *gDWS;           // backward
  char *fsync, *bsync;
  size_t fsync_bytes, bsync_bytes;
  // the regions' 256-byte headers (abort word, epoch, sticky failure bits), kept apart from the overlapping
  // forward / backward working sets: the forward region's header must survive the backward for the harvest
  char *fhdr, *bhdr;
  unsigned long long* stamps;  // diagnostic phase stamps (nullptr = off)
  float* dh;
  long lddh;
  const float* dlogp;
  float* logp;
};

struct Layout {
  size_t saved, fwd, bwd;
  bool overlay;  // the beam's shared layout keeps its post-combine buffers inside PC (carve)
};

// operands of the XCD-local decoder kernels (dec_xcd.inc)
struct XArgs {
  int U, nchains, allow_local, XLC, NCH;
  float* WX;    // (3S, A)  Wx' = [Wz_d; Wr_d; Wh_d] Wd_c Wc          (saved)
  float* WXT;   // (A, 3S)  Wx'^T                                    (saved)
  float* WXD;   // (3S, S)  [Wz_d; Wr_d; Wh_d] packed                (saved)
  float* WDC;   // (S, A)   Wd_c Wc                                  (fwd scratch)
  float* KX;    // (B*T, 3S) d-part constants of the gates            (fwd scratch)
  float* KD;    // (B*T, S)  Wd_c bc + Wd_y y_in + bd                 (fwd scratch)
  float* BKD;   // (S)       Wd_c bc + bd                             (fwd scratch)
  float* DE;    // (B*T, L)  de_{t,l}                                 (bwd scratch)
  float* DCS;   // (B*T, A)  dc_t (= AttnK::DC)                       (bwd scratch)
  float* VBAR;  // (B, Sc)   mean Vh row per utterance                 (bwd scratch)
  float* XWHT;  // (S, S)    Wh[:, :S]^T                               (saved)
  float* XZRT;  // (S, 2S)   [Wz[:, :S]; Wr[:, :S]]^T                   (saved)
  float* XWST;  // (S, Sc)   Ws^T                                      (saved)
  // prologue operand re-layouts (dec_xcd_pack_ops) so its GEMMs batch as NN problems (fwd scratch)
  float* PWDYT;  // (S, S)   Wd[:, S:]^T
  float* PWDCT;  // (S, S)   Wd[:, :S]^T
  float* PWCT;   // (A, S)   Wc^T
  float* PWXDT;  // (S, 3S)  WXD^T
  float* WDCT;   // (A, S)   (Wd_c Wc)^T
  // granule buffers, [2 slots][...]
  granule_t *gS, *gWS, *gPM, *gPL, *gPC, *gC, *gQ;     // forward (inside fsync)
  granule_t *gDGZ, *gDGR, *gDGH, *gDC, *gPDWS, *gDWS;  // backward (inside bsync)
  unsigned *fcensus, *bcensus;
  // sentinel rows of XCD-local chains (handoff.h), [T slots][B][...] floats, outside the zeroed regions
  float *sS, *sQ, *sC, *sWS;  // forward: s_t, q_t (S), c_t (A), ws_t (Sc)
  float *sDGZ, *sDGR, *sDGH, *sDC, *sDWS;  // backward: da_z, da_r, da_h (S), dc (A), dws (Sc)
};
// extra operands of the LSTM / hybrid kernels (carve, dec_xcd_lstm_prologue)
struct XLArgs {
  int S;          // real state width (the kernels carry SP)
  int hk, pl;     // hybrid taps kW and the left pad
  float* WG;      // (4SP, SP)  Wq_h, gate-major rows q SP + u, zero-padded             (saved)
  float* WXG;     // (4SP, A)   Wq_x Wd_c Wc, rows as WG                                 (saved)
  float* WSP;     // (Sc, SP)   Ws with zero columns past S                              (saved)
  float* WUT;     // (SP, 4SP)  WUT[n][q SP + u] = Wq_h[u][n]                            (saved)
  float* WXGT;    // (A, 4SP)   WXG^T                                                    (saved)
  float* WSTP;    // (SP, SCP)  Ws^T, zero-padded                                        (saved)
  float* WXD4;    // (4S, S)    [Wi_x; Wf_x; Wg_x; Wo_x] (the weight gradients' dd)      (saved)
  float* BQ;      // (4S)       bq_x + bq_h                                              (fwd scratch)
  float* KXG;     // (B T, 4SP) Wq_x KD_t + bq, zero-padded                              (fwd scratch)
  float* sS;      // [T][B][SP] s_t (chain-interleaved sentinel rows)                    (fwd)
  float* sDG[4];  // [T][B][SP] da_q (chain-interleaved)                                 (bwd)
  float* sDC[2];  // [T][B][A] the two K halves of dc                                    (bwd)
  float* sDWS;    // [T][B][SCP] dws (chain-interleaved; columns past Sc published as 0)  (bwd)
  granule_t *gS, *gE, *gA;  // [2][B][SP], [2][B][L] scores and alpha (hybrid location features)   (inside fsync)
  granule_t *gDG[4], *gDC[2], *gDWS, *gQA;  // [2][B][SP] x 4, [2][B][A] x 2, [2][B][SCP], [2][B][L][kW] (bsync)
  float* PDG;     // [B NX][kW][Sc] dG partials per (utterance, chunk)                   (bwd scratch)
};
constexpr int kXLC = 32;     // largest attention chunk (frames) of the XCD-local decoder, LDS-resident
constexpr int kXLCStream = 64;  // largest chunk when h / Vh rows are read from global memory each step
constexpr int kXMaxCh = 16;  // chunks per utterance
constexpr int kXChains = 8;  // chains per launch (one per XCD)
constexpr int kXWG = 32;     // workgroups per chain

// ---- XCD-local decoder (dec_xcd.inc) plan: chains of U utterances, one per XCD (U as small as
// 8 chains allow, so the attention work spreads over as many XCDs as possible), each utterance cut
// into NCH chunks of XLC frames (U * NCH <= 32 workgroups).  var = 0: the shape is served by the
// older kernels (S2S_DEC_MODE=persist / step force those).
struct XPlan {
  int var = 0, U = 0, nchains = 0, XLC = 0, NCH = 0, res = 1;
};
constexpr int kXlSP = 448, kXlSCP = 192;  // the LSTM kernels' padded S and Sc (var 3: S = 400, Sc = 160)

// Which decoder path serves a shape, resolved once per entry point by dec_route (attn_layout.inc); carve, the sync
// regions, the prologue, the forward, the backward, the weight gradients and the head predicates all read this.
enum DecPath { kPathSteps = 0, kPathPersist = 1, kPathXcd = 2, kPathXcdLstm = 3 };  // (tests/paths.py)
struct DecRoute {
  int path = kPathSteps;
  XPlan xp;           // the XCD-local plan (var = 0 off the two XCD paths)
  int pvar = 0;       // the persistent kernels' width variant (0 off the persist path)
  bool fold = false;  // the per-step path folds F4 + F5 / K4 + K5
  bool xcd() const { return path >= kPathXcd; }
};
}  // namespace
}  // namespace s2s
