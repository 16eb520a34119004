// The decoder's route (which path serves a shape) and its workspace layout; included by attn.hip at namespace scope.
namespace {
// S2S_DEC_MODE=step / persist (tests, A/B): force the per-step launches / the 7-seam persistent kernels; read once.
// s2s_debug_dec_mode(m) overrides it in-process (m = 0 auto, 1 step, 2 persist; -1 back to the environment's)
std::atomic<int> g_dec_mode_force{-1};
int dec_mode() {
  static const int m = [] {
    const char* e = std::getenv("S2S_DEC_MODE");
    return e && std::strcmp(e, "step") == 0 ? 1 : e && std::strcmp(e, "persist") == 0 ? 2 : 0;
  }();
  const int f = g_dec_mode_force.load();
  return f >= 0 ? f : m;
}
XPlan dec_xcd_plan(const AttnDims& d) {
  XPlan p;
  if (dec_mode() != 0) return p;
  int var = 0;
  if (d.lstm) {
    // the LSTM decoder with hybrid attention (dec_xcd_lstm.inc): the conv + BiLSTM model's shape (timit/timit.lua:
    // 127-155: S = 400, A = 256, scoreDepth 150 padded to 160, kW = 5), chains of <= 4 utterances, resident chunks
    if (d.hf > 0 && d.hk == 5 && d.S == 400 && d.A == 256 && d.Sc == 160) var = 3;
  } else if (d.hf == 0) {  // (hybrid attention with the GRU decoder: the per-step kernels)
    if (d.S == 256 && d.A == 512 && d.Sc == 512) var = 1;
    else if (d.S == 64 && d.A == 128 && d.Sc == 128) var = 2;
  }
  if (!var) return p;
  const int U = (d.B + kXChains - 1) / kXChains;
  if (U > 16 || (var == 3 && U > 4)) return p;
  const int nmax = std::min(kXMaxCh, kXWG / U);
  const int xlc = ((d.L + nmax - 1) / nmax + 3) / 4 * 4;
  if (xlc > kXLCStream || d.T > 256) return p;  // (dec_xcd_dvh stages up to 256 steps)
  // resident chunks while they fit LDS (U utterances x L frames x (A + Sc) floats per XCD); longer
  // utterances stream their h / Vh rows from global memory (L2 / MALL) every step
  // (S2S_DEC_STREAM = 1 / 0: force Vh-only / no residency -- diagnostics and the bitwise tests)
  const char* fs = std::getenv("S2S_DEC_STREAM");
  p.res = xlc <= kXLC ? 2 : 1;
  if (fs && std::strcmp(fs, "1") == 0) p.res = 1;
  if (fs && std::strcmp(fs, "0") == 0) p.res = 0;
  if (var == 3 && p.res != 2) return p;  // (the LSTM kernels keep their chunks resident)
  p.var = var;
  p.U = U;
  p.nchains = (d.B + U - 1) / U;
  p.XLC = xlc;
  p.NCH = (d.L + xlc - 1) / xlc;
  return p;
}

// The 7-seam persistent decoder kernels (attn_persist.inc): auto mode's fall-back where dec_xcd_plan declines a shape
// of the instantiated widths (B > 128, a chunk longer than 64 frames, T > 256), or forced by dec_mode() = 2;
// dec_mode() = 1 forces the per-step launches.
static int dec_persist_variant(const AttnDims& d) {
  if (dec_mode() == 1) return 0;
  if (d.hf > 0 || d.lstm) return 0;
  if (d.flen || d.tlen) return 0;  // variable-length batches: the XCD-local or the per-step kernels
  if ((d.L + LC - 1) / LC > 256) return 0;
  if (d.S == 256 && d.A == 512 && d.Sc == 512) return 1;
  if (d.S == 64 && d.A == 128 && d.Sc == 128) return 2;
  return 0;
}

// The one route decision: the XCD-local kernels where their plan takes the shape, else the persistent kernels where a
// variant fits (at launch time they may still find no co-resident candidate: DecCall::fwd_persist), else the steps.
DecRoute dec_route(const AttnDims& d) {
  DecRoute r;
  r.xp = dec_xcd_plan(d);
  r.pvar = r.xp.var ? 0 : dec_persist_variant(d);
  r.path = r.xp.var == 3 ? kPathXcdLstm : r.xp.var ? kPathXcd : r.pvar ? kPathPersist : kPathSteps;
  // The per-step path folds F4 + F5 (and K4 + K5) for the shapes only it serves: the LSTM decoder and hybrid attention
  // (the GRU content-attention per-step path stays bitwise equal to the persistent kernels of attn_persist.inc)
  r.fold = r.path == kPathSteps && (d.lstm || d.hf > 0);
  return r;
}

Layout carve(const AttnDims& d, AttnK* k, char* saved, char* scratch, XArgs* x = nullptr, XLArgs* y = nullptr) {
  const long B = d.B, L = d.L, T = d.T, A = d.A, Sc = d.Sc, S = d.S, O = d.O, M = d.M, Mk = (long)d.M * d.K;
  const long NCH = (d.L + LC - 1) / LC, BT = B * T;
  const bool beam = d.vh_rows > 0;  // the beam search's shared layout (AttnDims::vh_rows)
  Bump sv{saved, 0, 0};
  float* Vh = sv.take<float>((beam ? d.vh_rows : B) * L * Sc);
  float* WS = sv.take<float>(BT * Sc);
  float* E = sv.take<float>(BT * L);
  float* ALPHA = sv.take<float>(BT * L);
  float* LSE = sv.take<float>(BT);
  float* IND = sv.take<float>(BT);
  float* C = sv.take<float>(BT * A);
  float* HX = sv.take<float>(BT * 2 * S);
  const long NG = d.lstm ? 4 : 3;  // gate rows per step: GRU z, r, hh / LSTM i, f, g, o
  // The beam's shared layout: what a step writes only after dec_f3_combine has consumed the chunk partials PC
  // (F4 .. the MLP head: RHX, CY, the gates, U, the Maxout and the log-probabilities), and the search reads
  // before the next step's attention launch refills PC, lives inside PC when it fits there.
  const size_t ovl_counts[7] = {size_t(BT * 2 * S), size_t(BT * 2 * S), size_t(BT * NG * S), size_t(BT * M),
                                size_t(BT * M),     size_t(BT * O),     size_t(BT * Mk)};
  size_t ovl_bytes = 0;
  for (size_t n : ovl_counts) ovl_bytes = ((ovl_bytes + 255) & ~size_t(255)) + n * sizeof(float);
  const bool overlay = beam && ovl_bytes <= size_t(B * NCH * A) * sizeof(float);
  sv.lean = overlay;
  float* RHX = sv.take<float>(BT * 2 * S);
  float* CY = sv.take<float>(BT * 2 * S);
  float* GSV = sv.take<float>(BT * NG * S);
  sv.lean = false;
  float* VV = sv.take<float>(BT * (S + A));
  sv.lean = overlay;
  float* MM = sv.take<float>(BT * M);
  int* AM = sv.take<int>(BT * M);
  float* LOGP = sv.take<float>(BT * O);
  sv.lean = false;
  float* MASK = d.dropout > 0.f ? sv.take<float>(BT * (S + A)) : nullptr;
  sv.lean = beam;  // (the XCD-local kernels' operands: the beam steps are per-step launches)
  float* WX = sv.take<float>(3 * S * A);
  float* WXT = sv.take<float>(3 * S * A);
  float* WXD = sv.take<float>(3 * S * S);
  float* XWHT = sv.take<float>(S * S);
  float* XZRT = sv.take<float>(2 * S * S);
  float* XWST = sv.take<float>(S * Sc);
  float* VBAR = sv.take<float>(B * Sc);  // mean Vh row per utterance (computed by the forward)
  sv.lean = false;
  float* LW = d.lstm ? sv.take<float>(4 * S * 2 * S) : nullptr;
  float* LB = d.lstm ? sv.take<float>(4 * S) : nullptr;
  float* LCS = d.lstm ? sv.take<float>(BT * S) : nullptr;
  const long HK = d.hf > 0 ? d.hk : 0;
  float* HGT = HK ? sv.take<float>(HK * Sc) : nullptr;
  float* HCU = HK ? sv.take<float>(Sc) : nullptr;
  const XPlan xpl = dec_route(d).xp;
  const long NX = std::max(1, xpl.NCH);
  // the LSTM / hybrid XCD-local kernels' operands (var 3; empty otherwise)
  const bool v3 = xpl.var == 3 && !beam;
  const long SP = v3 ? kXlSP : 0, SCP = v3 ? kXlSCP : 0, S4 = v3 ? 4 * S : 0;
  float* lWG = sv.take<float>(4 * SP * SP);
  float* lWXG = sv.take<float>(4 * SP * A);
  float* lWSP = sv.take<float>(v3 ? Sc * SP : 0);
  float* lWUT = sv.take<float>(SP * 4 * SP);
  float* lWXGT = sv.take<float>(v3 ? A * 4 * SP : 0);
  float* lWSTP = sv.take<float>(SP * SCP);
  float* lWXD4 = sv.take<float>(S4 * (v3 ? S : 0));
  Bump f{scratch, 0, 0};
  float* PM = f.take<float>(B * NCH);
  float* PL = f.take<float>(B * NCH);
  float* PC = f.take<float>(B * NCH * A);
  f.lean = overlay;
  float* U = f.take<float>(BT * Mk);
  if (overlay) {
    Bump o{reinterpret_cast<char*>(PC), 0, 0};
    RHX = o.take<float>(ovl_counts[0]);
    CY = o.take<float>(ovl_counts[1]);
    GSV = o.take<float>(ovl_counts[2]);
    MM = o.take<float>(ovl_counts[3]);
    AM = o.take<int>(ovl_counts[4]);
    LOGP = o.take<float>(ovl_counts[5]);
    U = o.take<float>(ovl_counts[6]);
  }
  f.lean = beam;
  float* WDC = f.take<float>(S * A);
  float* PWDYT = f.take<float>(S * S);
  float* PWDCT = f.take<float>(S * S);
  float* PWCT = f.take<float>(A * S);
  float* PWXDT = f.take<float>(S * 3 * S);
  float* WDCT = f.take<float>(A * S);
  float* KX = f.take<float>(BT * 3 * S);
  float* KD = f.take<float>(BT * S);
  float* BKD = f.take<float>(S);
  float* lBQ = f.take<float>(S4);
  float* lKXG = f.take<float>(v3 ? BT * 4 * SP : 0);
  Bump g{scratch, 0, 0};
  g.lean = beam;
  float* DO = g.take<float>(BT * O);
  float* DU = g.take<float>(BT * Mk);
  float* DV = g.take<float>(BT * (S + A));
  float* DGA = g.take<float>(BT * NG * S);
  float* DS = g.take<float>(B * S);
  float* DSP = g.take<float>(B * S);
  float* DSPF = g.take<float>(B * S);
  float* DD = g.take<float>(BT * S);
  float* DCY = g.take<float>(BT * 2 * S);
  float* DC = g.take<float>(BT * A);
  float* DVH = g.take<float>(B * L * Sc);
  float* PDWS = g.take<float>(B * NCH * Sc);
  float* DWS = g.take<float>(BT * Sc);
  float* DWEACC = g.take<float>(B * NCH * Sc);
  float* YP = g.take<float>(BT * O);
  float* WhT = g.take<float>(S * S);
  float* GT = g.take<float>(2 * S * NG * S);
  float* LDW = d.lstm ? g.take<float>(4 * S * 2 * S) : nullptr;
  float* WdT = g.take<float>(2 * S * S);
  float* WcT = g.take<float>(A * S);
  float* WsT = g.take<float>(S * Sc);
  float* DE = g.take<float>(BT * L);

  float* QA = HK ? g.take<float>(2 * B * L * HK) : nullptr;
  float* PDG = HK ? g.take<float>(B * NCH * HK * Sc) : nullptr;
  float* DGT = HK ? g.take<float>(HK * Sc) : nullptr;
  float* DCU = HK ? g.take<float>(Sc) : nullptr;
  // granule regions (256-byte header = abort word), zeroed by one memset before each persistent launch
  char* fsync = f.take<char>(256);
  granule_t* gS = f.take<granule_t>(2 * B * S);
  granule_t* gWS = f.take<granule_t>(2 * B * Sc);
  granule_t* gPM = f.take<granule_t>(2 * B * NCH);
  granule_t* gPL = f.take<granule_t>(2 * B * NCH);
  granule_t* gPC = f.take<granule_t>(2 * B * NCH * A);
  granule_t* gC = f.take<granule_t>(2 * B * A);
  granule_t* gCY = f.take<granule_t>(2 * B * 2 * S);
  granule_t* gD = f.take<granule_t>(2 * B * S);
  granule_t* gQ = f.take<granule_t>(2 * B * S);
  granule_t* xgS = f.take<granule_t>(2 * B * S);
  granule_t* xgWS = f.take<granule_t>(2 * B * Sc);
  granule_t* xgPM = f.take<granule_t>(2 * B * NX);
  granule_t* xgPL = f.take<granule_t>(2 * B * NX);
  granule_t* xgPC = f.take<granule_t>(2 * B * NX * A);
  granule_t* xgC = f.take<granule_t>(2 * B * A);
  granule_t* xgQ = f.take<granule_t>(2 * B * S);
  granule_t* lgS = f.take<granule_t>(2 * B * SP);
  granule_t* lgE = f.take<granule_t>(v3 ? 2 * B * L : 0);
  granule_t* lgA = f.take<granule_t>(v3 ? 2 * B * L : 0);
  unsigned* fcensus = f.take<unsigned>(kXChains * kXWG);
  const size_t fsync_bytes = fsync ? f.off - (size_t)(fsync - scratch) : 0;
  float* lsS = f.take<float>(BT * SP);
  float* xsS = f.take<float>(BT * S);
  float* xsQ = f.take<float>(BT * S);
  float* xsC = f.take<float>(BT * A);
  float* xsWS = f.take<float>(BT * Sc);
  char* bsync = g.take<char>(256);
  granule_t* gZ = g.take<granule_t>(2 * B * S);
  granule_t* gR = g.take<granule_t>(2 * B * S);
  granule_t* gH = g.take<granule_t>(2 * B * S);
  granule_t* gDD = g.take<granule_t>(2 * B * S);
  granule_t* gDCY = g.take<granule_t>(2 * B * S);
  granule_t* gDC = g.take<granule_t>(2 * B * A);
  granule_t* gPDWS = g.take<granule_t>(2 * B * NCH * Sc);
  granule_t* gDWS = g.take<granule_t>(2 * B * Sc);
  granule_t* xgDGZ = g.take<granule_t>(2 * B * S);
  granule_t* xgDGR = g.take<granule_t>(2 * B * S);
  granule_t* xgDGH = g.take<granule_t>(2 * B * S);
  granule_t* xgDC = g.take<granule_t>(2 * B * A);
  granule_t* xgPDWS = g.take<granule_t>(2 * B * NX * Sc);
  granule_t* xgDWS = g.take<granule_t>(2 * B * Sc);
  granule_t* lgDG[4];
  for (auto& q : lgDG) q = g.take<granule_t>(2 * B * SP);
  granule_t* lgDC[2];
  for (auto& q : lgDC) q = g.take<granule_t>(v3 ? 2 * B * A : 0);
  granule_t* lgDWS = g.take<granule_t>(2 * B * SCP);
  granule_t* lgQA = g.take<granule_t>(v3 ? 2 * B * L * HK : 0);
  unsigned* bcensus = g.take<unsigned>(kXChains * kXWG);
  const size_t bsync_bytes = bsync ? g.off - (size_t)(bsync - scratch) : 0;
  float* lsDG[4];
  for (auto& q : lsDG) q = g.take<float>(BT * SP);
  float* lsDC[2];
  for (auto& q : lsDC) q = g.take<float>(v3 ? BT * A : 0);
  float* lsDWS = g.take<float>(BT * SCP);
  float* lPDG = g.take<float>(v3 ? B * NX * HK * Sc : 0);
  float* xsDGZ = g.take<float>(BT * S);
  float* xsDGR = g.take<float>(BT * S);
  float* xsDGH = g.take<float>(BT * S);
  float* xsDC = g.take<float>(BT * A);
  float* xsDWS = g.take<float>(BT * Sc);
  if (k) {
    k->gS = gS; k->gWS = gWS; k->gPM = gPM; k->gPL = gPL; k->gPC = gPC; k->gC = gC; k->gCY = gCY; k->gD = gD;
    k->gQ = gQ; k->gZ = gZ; k->gR = gR; k->gH = gH; k->gDD = gDD; k->gDCY = gDCY; k->gDC = gDC; k->gPDWS = gPDWS;
    k->gDWS = gDWS; k->fsync = fsync; k->bsync = bsync; k->fsync_bytes = fsync_bytes; k->bsync_bytes = bsync_bytes;
    k->B = d.B; k->L = d.L; k->T = d.T; k->A = d.A; k->Sc = d.Sc; k->S = d.S; k->O = d.O; k->M = d.M; k->K = d.K;
    k->NCH = (int)NCH; k->penalty = d.penalty; k->t = 0;
    k->flen = d.flen; k->tlen = d.tlen;
    k->hk = (int)HK; k->hf = d.hf;
    k->lstm = d.lstm; k->LW = LW; k->LB = LB; k->LC = LCS; k->LDW = LDW;
    k->HGT = HGT; k->HCU = HCU; k->QA = QA; k->PDG = PDG; k->DGT = DGT; k->DCU = DCU;
    k->MASK = MASK;
    k->Vh = Vh; k->WS = WS; k->E = E; k->ALPHA = ALPHA; k->LSE = LSE; k->IND = IND; k->C = C; k->HX = HX;
    k->RHX = RHX; k->CY = CY; k->GSV = GSV; k->VV = VV; k->MM = MM; k->AM = AM; k->LOGP = LOGP;
    k->PM = PM; k->PL = PL; k->PC = PC; k->U = U;
    k->DO = DO; k->DU = DU; k->DV = DV; k->DGA = DGA; k->DS = DS; k->DSP = DSP; k->DSPF = DSPF; k->DD = DD;
    k->DCY = DCY; k->DC = DC; k->DVH = DVH; k->PDWS = PDWS; k->DWS = DWS; k->DWEACC = DWEACC; k->YP = YP;
    k->WhT = WhT; k->GT = GT; k->WdT = WdT; k->WcT = WcT; k->WsT = WsT;
  }
  if (x) {
    x->WX = WX; x->WXT = WXT; x->WXD = WXD; x->WDC = WDC; x->KX = KX; x->KD = KD; x->BKD = BKD; x->DE = DE;
    x->DCS = DC; x->VBAR = VBAR; x->XWHT = XWHT; x->XZRT = XZRT; x->XWST = XWST;
    x->PWDYT = PWDYT; x->PWDCT = PWDCT; x->PWCT = PWCT; x->PWXDT = PWXDT; x->WDCT = WDCT;
    x->gS = xgS; x->gWS = xgWS; x->gPM = xgPM; x->gPL = xgPL; x->gPC = xgPC; x->gC = xgC; x->gQ = xgQ;
    x->gDGZ = xgDGZ; x->gDGR = xgDGR; x->gDGH = xgDGH; x->gDC = xgDC; x->gPDWS = xgPDWS; x->gDWS = xgDWS;
    x->fcensus = fcensus; x->bcensus = bcensus;
    x->sS = xsS; x->sQ = xsQ; x->sC = xsC; x->sWS = xsWS;
    x->sDGZ = xsDGZ; x->sDGR = xsDGR; x->sDGH = xsDGH; x->sDC = xsDC; x->sDWS = xsDWS;
  }
  if (y) {
    y->S = d.S; y->hk = (int)HK; y->pl = HK ? (HK % 2 ? (int)(HK - 1) / 2 : (int)HK / 2) : 0;
    y->WG = lWG; y->WXG = lWXG; y->WSP = lWSP; y->WUT = lWUT; y->WXGT = lWXGT; y->WSTP = lWSTP; y->WXD4 = lWXD4;
    y->BQ = lBQ; y->KXG = lKXG; y->sS = lsS; y->gS = lgS; y->gE = lgE; y->gA = lgA;
    for (int q = 0; q < 4; ++q) { y->sDG[q] = lsDG[q]; y->gDG[q] = lgDG[q]; }
    for (int q = 0; q < 2; ++q) { y->sDC[q] = lsDC[q]; y->gDC[q] = lgDC[q]; }
    y->sDWS = lsDWS; y->gDWS = lgDWS; y->gQA = lgQA; y->PDG = lPDG;
  }
  if (k && scratch) {  // headers behind the GEMM slabs (attn_scratch_bytes)
    const size_t hoff = ((std::max(f.off + 256, g.off + 256) + 255) & ~size_t(255)) + sizeof(float) * kGemmWsFloats;
    k->fhdr = scratch + hoff;
    k->bhdr = scratch + hoff + 256;
  }
  return Layout{sv.off + 256, f.off + 256, g.off + 256, overlay};
}

}  // namespace

size_t attn_saved_bytes(const AttnDims& d) { return carve(d, nullptr, nullptr, nullptr).saved; }
// scratch = [forward | backward working sets (overlapping)] + split-K slabs of the GEMMs
static size_t attn_ws_offset(const AttnDims& d) {
  Layout l = carve(d, nullptr, nullptr, nullptr);
  return ((l.fwd > l.bwd ? l.fwd : l.bwd) + 255) & ~size_t(255);
}
// + the two sync-region headers (carve: fhdr, bhdr)
size_t attn_scratch_bytes(const AttnDims& d) { return attn_ws_offset(d) + sizeof(float) * kGemmWsFloats + 512; }
static GemmWs attn_gemm_ws(const AttnDims& d, void* scratch) {
  return GemmWs{reinterpret_cast<float*>(static_cast<char*>(scratch) + attn_ws_offset(d)), kGemmWsFloats};
}
// the saved buffer's views (no scratch: the scratch pointers of the result are offsets from null)
static AttnK saved_view(const AttnDims& d, const void* saved) {
  AttnK k{};
  carve(d, &k, (char*)saved, nullptr);
  return k;
}
const float* attn_saved_mlp_input(const AttnDims& d, const void* saved) { return saved_view(d, saved).VV; }
const float* attn_saved_alpha(const AttnDims& d, const void* saved) { return saved_view(d, saved).ALPHA; }
const float* attn_saved_ws(const AttnDims& d, const void* saved) { return saved_view(d, saved).WS; }
const float* attn_saved_vh(const AttnDims& d, const void* saved) { return saved_view(d, saved).Vh; }
const float* attn_saved_mono_ind(const AttnDims& d, const void* saved) { return saved_view(d, saved).IND; }
const int* attn_saved_maxout_argmax(const AttnDims& d, const void* saved) { return saved_view(d, saved).AM; }
const float* attn_saved_dropout_mask(const AttnDims& d, const void* saved) { return saved_view(d, saved).MASK; }
