// ================================================================== beam search
// Attention:BeamSearch (Attention.lua:332-438) for B utterances at once, all on the device.  The
// K hypotheses of every utterance are R = B*K rows of the per-step decoder kernels run as a T = 2
// problem: row t = 1 of each is the decode step, its s_{t-1} and y_{t-1} written by beam_prep into
// the t = 1 slots (HX[:, :S], labels[:, 0]; label -1 = zeros_y at the first step).  beam_update then
// does the reference's bookkeeping per utterance: p_next = logp + p_beam over the active hypotheses,
// torch.topk(K) of the flattened candidates (sorted; ties -> lower index), the first K - finished of
// them extend their parent (finished on eos or at maxseqlength), states gathered from the parents.
namespace {

struct BeamK {
  int B, K, maxlen, eos, S, O, L, hyb, lstm;
  int *nact, *nfin, *done;
  int *yprev, *hist, *hlen, *fseq, *flen, *lab2;
  // per hypothesis, double-buffered by step parity: decoder state s, attention alpha (hybrid attention's
  // location features read alpha_{t-1}) and the LSTM cell (mem) -- the reference's hidden {alpha, s, mem}
  // (Attention.lua:360-403)
  float *pbeam, *s, *fscore, *alpha, *mem;
  float* mlp_in;  // (R, S + A) decoder_mlp input rows of the current step (external decoder_mlp)
  int* maxlens;   // (B) each utterance's own hypothesis length limit, in [1, maxlen]
  // shared-annotation path (beam_f2_shared): the caller's h (B, L, A), kept in the state by beam_init because
  // the stepwise calls do not pass it again, and the utterances' frame lengths (B, or null)
  const float** hptr;
  const int* frames;
};

constexpr int kBeamMaxK = 16;

// The attention chunk of dec_f2_attn for all active hypotheses of one utterance at once.  grid (NCH, B).
// Row r = b*K + j (j < nact[b]) of the T = 2 problem scores utterance b's Vh rows against its own ws and sums
// its own context, but every Vh / h frame row is loaded once per workgroup: the Vh float4 of a lane meets all
// hypotheses' ws before the next one is fetched, and the context loop's hv[LC] registers are reused per row.
// Per (row, frame) the sums run in dec_f2_attn's order (lane-strided float4 columns, wave_sum, context in
// frame order).  Frames l >= L_b score -inf and weigh 0; a chunk wholly past L_b writes PM = -inf, PL = PC = 0.
// HYB (hybrid location-aware attention): what stays per hypothesis is ws and alpha_{t-1}.  The chunk's alpha_{t-1}
// halo of every active row (the row's t = 0 ALPHA slot, filled by beam_prep; 0 outside [0, L), as hyb_stage_alpha
// stages one row's) waits in LDS, and a lane's HCU and tap float4s of HGT are loaded once for all hypotheses.  Per
// (row, frame): u = HCU + sum_i HGT_i apl[j][li + i] (taps in order, hyb_uf4_lds), z = (ws_j + Vh) + u, as
// dec_f2_attn forms them.  alpha is 0 past L_b (E = -inf there), so the halo reads the zero padding the reference
// applies to an utterance of L_b frames.
template <int WV, bool HYB>
__global__ __launch_bounds__(64 * WV) void beam_f2_shared(AttnK k, BeamK q) {
  constexpr int FPW = LC / WV, NT = 64 * WV;
  __shared__ float sc[kBeamMaxK][LC];
  __shared__ float pw[kBeamMaxK][LC];
  __shared__ float apl[HYB ? kBeamMaxK : 1][LC + kMaxHybK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ch = blockIdx.x, b = blockIdx.y;
  if (q.done[b]) return;
  const int L = k.L, Sc = k.Sc, A = k.A, K = q.K, NCH = k.NCH;
  const int na = min(q.nact[b], K);
  const int Lb = q.frames ? min(q.frames[b], L) : L;
  const float* we = k.P.we;
  const float* ws0 = k.WS + ((long)b * K * 2 + 1) * Sc;  // row r's ws_t at ws0 + j * 2 * Sc (t = 1 of T = 2)
  const int kw = HYB ? min(k.hk, kMaxHybK) : 0;
  if constexpr (HYB) {
    const int pl = hyb_pad_left(kw), n = LC + kw - 1;
    for (int x = tid; x < na * n; x += NT) {
      const int j = x / n, i = x - j * n, m = ch * LC + i - pl;
      apl[j][i] = (m >= 0 && m < L) ? k.ALPHA[((long)(b * K + j) * 2) * L + m] : 0.f;
    }
    __syncthreads();
  }
  for (int i = 0; i < FPW; ++i) {
    const int li = wave * FPW + i, l = ch * LC + li;
    float part[kBeamMaxK];
#pragma unroll
    for (int j = 0; j < kBeamMaxK; ++j) part[j] = 0.f;
    if (l < Lb) {
      const float* vh = k.Vh + ((long)b * L + l) * Sc;
      for (int c4 = lane; c4 < Sc / 4; c4 += 64) {
        const float4 v = reinterpret_cast<const float4*>(vh)[c4];
        const float4 e = reinterpret_cast<const float4*>(we)[c4];
        if constexpr (HYB) {
          const float4 hc = reinterpret_cast<const float4*>(k.HCU)[c4];
          float4 g[kMaxHybK];
#pragma unroll
          for (int i = 0; i < kMaxHybK; ++i)
            g[i] = i < kw ? reinterpret_cast<const float4*>(k.HGT + (long)i * Sc)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int j = 0; j < kBeamMaxK; ++j) {
            if (j < na) {
              const float4 w = reinterpret_cast<const float4*>(ws0 + (long)j * 2 * Sc)[c4];
              float4 z = make_float4(w.x + v.x, w.y + v.y, w.z + v.z, w.w + v.w);
              float4 u = hc;
#pragma unroll
              for (int i = 0; i < kMaxHybK; ++i) {
                if (i < kw) {
                  const float a = apl[j][li + i];
                  u.x += g[i].x * a; u.y += g[i].y * a; u.z += g[i].z * a; u.w += g[i].w * a;
                }
              }
              z.x += u.x; z.y += u.y; z.z += u.z; z.w += u.w;
              part[j] += e.x * tanhf(z.x) + e.y * tanhf(z.y) + e.z * tanhf(z.z) + e.w * tanhf(z.w);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < kBeamMaxK; ++j) {
            if (j < na) {
              const float4 w = reinterpret_cast<const float4*>(ws0 + (long)j * 2 * Sc)[c4];
              const float4 z = make_float4(w.x + v.x, w.y + v.y, w.z + v.z, w.w + v.w);
              part[j] += e.x * tanhf(z.x) + e.y * tanhf(z.y) + e.z * tanhf(z.z) + e.w * tanhf(z.w);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kBeamMaxK; ++j) {
      if (j < na) {
        const float p = wave_sum(part[j]);
        if (lane == 0) sc[j][li] = l < Lb ? p : -INFINITY;
      }
    }
  }
  __syncthreads();
  if (tid < na * LC) {
    const int j = tid / LC, li = tid - j * LC, l = ch * LC + li;
    float m = -INFINITY;
    for (int i = 0; i < LC; ++i) m = fmaxf(m, sc[j][i]);
    pw[j][li] = l < Lb ? expf(sc[j][li] - m) : 0.f;
    if (l < L) k.E[((long)(b * K + j) * 2 + 1) * L + l] = sc[j][li];
    if (li == 0) k.PM[(b * K + j) * NCH + ch] = m;
  }
  __syncthreads();
  if (tid < na) {
    float s = 0.f;
    for (int i = 0; i < LC; ++i) s += pw[tid][i];
    k.PL[(b * K + tid) * NCH + ch] = s;
  }
  const float* h = q.hptr[0];
  const int lend = min(LC, L - ch * LC);
  for (int a4 = tid; a4 < A / 4; a4 += NT) {
    float4 hv[LC];
#pragma unroll
    for (int i = 0; i < LC; ++i)
      hv[i] = i < lend ? reinterpret_cast<const float4*>(h + ((long)b * L + ch * LC + i) * A)[a4]
                       : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < na; ++j) {
      float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < LC; ++i) {
        if (i < lend) {
          const float p = pw[j][i];
          acc.x += p * hv[i].x; acc.y += p * hv[i].y; acc.z += p * hv[i].z; acc.w += p * hv[i].w;
        }
      }
      reinterpret_cast<float4*>(k.PC + ((long)(b * K + j) * NCH + ch) * A)[a4] = acc;
    }
  }
}

// hypothesis row r = b*K + k gets utterance b's annotations (grid.y = utterance)
__global__ void beam_rep_h(const float* h, float* hr, int K, long per) {
  const int b = blockIdx.y;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (long)K * per; i += (long)gridDim.x * blockDim.x)
    hr[(long)b * K * per + i] = h[(long)b * per + i % per];
}

__global__ void beam_init(BeamK q, const float* h) {
  const int R = q.B * q.K;
  if (blockIdx.x == 0 && threadIdx.x == 0) q.hptr[0] = h;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < R * q.S; i += gridDim.x * blockDim.x) {
    q.s[i] = 0.f;
    if (q.lstm) q.mem[i] = 0.f;
  }
  if (q.hyb)
    for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < (long)R * q.L; i += gridDim.x * blockDim.x) q.alpha[i] = 0.f;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
    q.pbeam[r] = 0.f;
    q.yprev[r] = -1;
    q.hlen[r] = 0;
    q.flen[r] = 0;
    if (r < q.B) {
      q.nact[r] = 1;
      q.nfin[r] = 0;
      q.done[r] = 0;
      q.maxlens[r] = q.maxlen;
    }
  }
}

// s_{t-1} and y_{t-1} of every hypothesis row into the t = 1 slots of the T = 2 problem; alpha_{t-1} (hybrid)
// and the LSTM cell c_{t-1} into its t = 0 slots (what the step kernels read as the previous step's)
__global__ void beam_prep(AttnK k, BeamK q, int par) {
  const int R = q.B * q.K, S = q.S, L = q.L;
  const float* s = q.s + (long)par * R * S;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < R * S; i += gridDim.x * blockDim.x) {
    const int r = i / S, n = i - r * S;
    k.HX[((long)r * 2 + 1) * 2 * S + n] = s[i];
    if (q.lstm) k.LC[((long)r * 2) * S + n] = q.mem[(long)par * R * S + i];
  }
  if (q.hyb)
    for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < (long)R * L; i += gridDim.x * blockDim.x) {
      const long r = i / L, l = i - r * L;
      k.ALPHA[(r * 2) * L + l] = q.alpha[(long)par * R * L + i];
    }
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
    q.lab2[2 * r] = q.yprev[r];
    q.lab2[2 * r + 1] = 0;
  }
}

// each utterance's own limit (s2s_attn_beam_set_maxlens), clamped to [1, maxlen]
__global__ void beam_set_maxlens(BeamK q, const int* maxlens) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < q.B; b += gridDim.x * blockDim.x)
    q.maxlens[b] = min(max(maxlens[b], 1), q.maxlen);
}

__global__ __launch_bounds__(256) void beam_update(AttnK k, BeamK q, int count) {
  __shared__ float bv[256];
  __shared__ int bi[256];
  __shared__ int sel[kBeamMaxK];
  __shared__ float selv[kBeamMaxK];
  __shared__ int fpar[kBeamMaxK], ftok[kBeamMaxK], fdst[kBeamMaxK], npar[kBeamMaxK], ntok[kBeamMaxK];
  __shared__ float fsc[kBeamMaxK], np_[kBeamMaxK];
  __shared__ int nf_new, nn_new;
  const int b = blockIdx.x, tid = threadIdx.x, K = q.K, O = q.O, S = q.S, R = q.B * K;
  if (q.done[b]) return;
  const int nact = q.nact[b], ncand = nact * O;
  const int par = count & 1, nxt = par ^ 1, maxlen = q.maxlens[b];  // the utterance's own limit
  auto cval = [&](int c) {
    const int i = c / O, j = c - i * O;
    return k.LOGP[((long)(b * K + i) * 2 + 1) * O + j] + q.pbeam[b * K + i];
  };
  // torch.topk(p_next, K, 1, true): K rounds of a block arg-max over the unselected candidates
  const int nsel = min(K, ncand);
  for (int m = 0; m < nsel; ++m) {
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c = tid; c < ncand; c += 256) {
      bool taken = false;
      for (int p = 0; p < m; ++p) taken = taken || sel[p] == c;
      if (taken) continue;
      const float v = cval(c);
      if (v > best || (v == best && c < bidx)) { best = v; bidx = c; }
    }
    bv[tid] = best;
    bi[tid] = bidx;
    __syncthreads();
    if (tid == 0) {
      float bb = bv[0];
      int ii = bi[0];
      for (int x = 1; x < 256; ++x)
        if (bv[x] > bb || (bv[x] == bb && bi[x] < ii)) { bb = bv[x]; ii = bi[x]; }
      sel[m] = ii;
      selv[m] = bb;
    }
    __syncthreads();
  }
  // the first K - finished of the sorted candidates extend their parents (Attention.lua:413-430); at
  // count 0 the one zero-state row offers all K (:369-387), later the K - finished survivors
  if (tid == 0) {
    int nf = 0, nn = 0;
    const int fin = q.nfin[b];
    for (int m = 0; m < K - fin && m < nsel; ++m) {
      const int i = sel[m] / O, j = sel[m] - i * O;
      if (j == q.eos || (count > 0 && count == maxlen)) {
        fpar[nf] = i; ftok[nf] = j; fsc[nf] = selv[m]; fdst[nf] = fin + nf; ++nf;
      } else {
        npar[nn] = i; ntok[nn] = j; np_[nn] = selv[m]; ++nn;
      }
    }
    nf_new = nf;
    nn_new = nn;
  }
  __syncthreads();
  const int nf = nf_new, nn = nn_new, L1 = q.maxlen + 1;
  const int* hcur = q.hist + (long)par * R * L1;
  int* hnew = q.hist + (long)nxt * R * L1;
  const int* lcur = q.hlen + par * R;
  int* lnew = q.hlen + nxt * R;
  for (int f = 0; f < nf; ++f) {  // finished hypotheses: parent's tokens + the final token
    const int src = b * K + fpar[f], dst = b * K + fdst[f], len = lcur[src];
    for (int x = tid; x < len; x += 256) q.fseq[(long)dst * L1 + x] = hcur[(long)src * L1 + x];
    if (tid == 0) {
      q.fseq[(long)dst * L1 + len] = ftok[f];
      q.flen[dst] = len + 1;
      q.fscore[dst] = fsc[f];
    }
  }
  float* snew = q.s + (long)nxt * R * S;
  for (int e = 0; e < nn; ++e) {  // surviving hypotheses: gather tokens and the decoder state of the parent
    const int src = b * K + npar[e], dst = b * K + e, len = lcur[src];
    for (int x = tid; x < len; x += 256) hnew[(long)dst * L1 + x] = hcur[(long)src * L1 + x];
    const float* sv = k.VV + ((long)src * 2 + 1) * (S + k.A);
    for (int n = tid; n < S; n += 256) snew[(long)dst * S + n] = sv[n];
    if (q.lstm)
      for (int n = tid; n < S; n += 256)
        q.mem[(long)nxt * R * S + (long)dst * S + n] = k.LC[((long)src * 2 + 1) * S + n];
    if (q.hyb)
      for (int l = tid; l < q.L; l += 256)
        q.alpha[(long)nxt * R * q.L + (long)dst * q.L + l] = k.ALPHA[((long)src * 2 + 1) * q.L + l];
    if (tid == 0) {
      hnew[(long)dst * L1 + len] = ntok[e];
      lnew[dst] = len + 1;
      q.pbeam[dst] = np_[e];
      q.yprev[dst] = ntok[e];
    }
  }
  if (tid == 0) {
    q.nfin[b] += nf;
    q.nact[b] = nn;
    q.done[b] = (q.nfin[b] >= K || count >= maxlen) ? 1 : 0;
  }
}

// external decoder_mlp: the step's [s_t; c_t] rows (t = 1 slots) out, the caller's log-probabilities in
__global__ void beam_mlp_rows(AttnK k, BeamK q) {
  const int R = q.B * q.K, W = q.S + k.A;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (long)R * W; i += (long)gridDim.x * blockDim.x) {
    const long r = i / W, c = i - r * W;
    q.mlp_in[i] = k.VV[(r * 2 + 1) * W + c];
  }
}
__global__ void beam_put_logp(AttnK k, BeamK q, const float* logp) {
  const int R = q.B * q.K, O = q.O;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (long)R * O; i += (long)gridDim.x * blockDim.x) {
    const long r = i / O, o = i - r * O;
    k.LOGP[(r * 2 + 1) * O + o] = logp[i];
  }
}

// prediction = y_finished[argmax p_finished] (first maximum)
__global__ void beam_final(BeamK q, int* out, int ldo, int* out_len, float* out_score) {
  const int b = blockIdx.x, K = q.K, L1 = q.maxlen + 1;
  __shared__ int best;
  if (threadIdx.x == 0) {
    int bi = 0;
    float bs = -INFINITY;
    for (int f = 0; f < q.nfin[b]; ++f)
      if (q.fscore[b * K + f] > bs) { bs = q.fscore[b * K + f]; bi = f; }
    best = bi;
    out_len[b] = q.nfin[b] > 0 ? q.flen[b * K + bi] : 0;
    if (out_score) out_score[b] = bs;
  }
  __syncthreads();
  const int len = q.nfin[b] > 0 ? q.flen[b * K + best] : 0;
  for (int x = threadIdx.x; x < ldo; x += blockDim.x)
    out[(long)b * ldo + x] = x < len ? q.fseq[((long)b * K + best) * L1 + x] : -1;
}

// WagnerFischer (utils.lua:3-27): Levenshtein distance of one sequence pair per block
__global__ void edit_distance_kernel(int n, const int* a, const int* alen, int lda, const int* b, const int* blen,
                                     int ldb, int* out) {
  extern __shared__ int row[];
  const int p = blockIdx.x;
  if (p >= n || threadIdx.x != 0) return;
  const int m = alen[p], nb = blen[p];
  const int* x = a + (long)p * lda;
  const int* y = b + (long)p * ldb;
  for (int i = 0; i <= m; ++i) row[i] = i;  // column j = 0: d[i][0] = i
  for (int j = 1; j <= nb; ++j) {
    int diag = row[0];
    row[0] = j;
    for (int i = 1; i <= m; ++i) {
      const int up = row[i];
      row[i] = x[i - 1] == y[j - 1] ? diag : min(min(up + 1, row[i - 1] + 1), diag + 1);
      diag = up;
    }
  }
  out[p] = row[m];
}

// s2s_debug_beam_replicate(1): content attention also takes the replicated path (A/B arm, tests); a search must
// run start to end under one setting, since the workspace layout follows it
std::atomic<int> g_beam_replicate{0};
// Content attention shares each utterance's Vh and h among its hypotheses (beam_f2_shared); hybrid attention does
// when the caller opts in (AttnDims::share_hybrid: only ws and alpha_{t-1} are per hypothesis) and otherwise keeps
// one private copy per hypothesis row
bool beam_shared(const AttnDims& d) { return (d.hf == 0 || d.share_hybrid) && !g_beam_replicate.load(); }

AttnDims beam_dims(const AttnDims& d, int K) {
  AttnDims d2 = d;
  d2.vh_rows = beam_shared(d) ? d.B : 0;
  d2.B = d.B * K;
  d2.T = 2;
  d2.dropout = 0.f;  // evaluate() mode
  d2.dropout_mask = nullptr;
  d2.flen = nullptr;  // rows are hypotheses; every utterance's annotations are searched whole
  d2.tlen = nullptr;
  return d2;
}

struct BeamLayout {
  size_t hrep, saved, scratch, state, fstate, total;
};
BeamLayout beam_layout(const AttnDims& d, int K, int maxlen) {
  const AttnDims d2 = beam_dims(d, K);
  const size_t R = (size_t)d.B * K, L1 = (size_t)maxlen + 1;
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  BeamLayout l;
  const bool shared = d2.vh_rows > 0;
  l.hrep = 0;
  l.saved = shared ? 0 : up(sizeof(float) * R * d.L * d.A);  // (the shared path reads the caller's h)
  l.scratch = l.saved + up(attn_saved_bytes(d2));
  l.state = l.scratch + up(attn_scratch_bytes(d2));
  const size_t ints = 2 /*hptr*/ + 4 * (size_t)d.B + R /*yprev*/ + 2 * R * L1 /*hist*/ + 2 * R /*hlen*/ +
                      R * L1 /*fseq*/ + R /*flen*/ + 2 * R /*lab2*/;
  // alpha_{t-1} per hypothesis only feeds hybrid attention's location features: the shared content layout has none
  // (the LSTM cell only with an LSTM decoder)
  const size_t floats = R /*pbeam*/ + 2 * R * d.S /*s*/ + R /*fscore*/ +
                        (shared && d.hf == 0 ? 0 : 2 * R * d.L) /*alpha*/ +
                        (d.lstm ? 2 * R * d.S : 0) /*mem*/ + R * (size_t)(d.S + d.A) /*mlp_in*/;
  l.fstate = l.state + up(4 * ints);
  l.total = l.fstate + up(4 * floats);
  return l;
}

}  // namespace

size_t attn_beam_workspace_bytes(const AttnDims& d, int K, int maxlen) { return beam_layout(d, K, maxlen).total; }

// The beam's device state inside the workspace (beam_layout): the T = 2 decoder problem of R = B*K rows and
// the per-hypothesis bookkeeping.  Every stage re-derives the same views from (d, K, maxlen, ws).
struct BeamView {
  AttnDims d2;
  bool overlay;
  AttnK k;
  BeamK q;
  float* hrep;
  GemmWs gws;
};
static int beam_view(const AttnDims& d, const AttnParams& P, int eos, int K, int maxlen, void* ws, size_t ws_bytes,
                     BeamView& v) {
  S2S_TRY(attn_check_dims(d));
  S2S_REQUIRE(K >= 1 && K <= kBeamMaxK && K <= d.O, "beam search: K must be in [1, 16] and <= outputDepth");
  S2S_REQUIRE(maxlen >= 1 && eos >= 0 && eos < d.O, "beam search: bad eos / maxlen");
  S2S_REQUIRE(!d.flen || d.hf == 0 || d.share_hybrid,
              "beam search: frame lengths unsupported with hybrid attention unless beam_share_hybrid is set "
              "(search an utterance's own frames)");
  S2S_REQUIRE(!d.flen || beam_shared(d), "beam search: frame lengths need the shared-annotation path");
  const BeamLayout bl = beam_layout(d, K, maxlen);
  S2S_REQUIRE(ws && ws_bytes >= bl.total, "beam search: workspace too small");
  v.d2 = beam_dims(d, K);
  char* base = static_cast<char*>(ws);
  v.hrep = reinterpret_cast<float*>(base + bl.hrep);
  v.k = AttnK{};
  v.overlay = carve(v.d2, &v.k, base + bl.saved, base + bl.scratch).overlay;
  const int B = d.B, R = B * K, S = d.S, L1 = maxlen + 1;
  BeamK& q = v.q;
  q = BeamK{};
  q.B = B; q.K = K; q.maxlen = maxlen; q.eos = eos; q.S = S; q.O = d.O; q.L = d.L;
  q.hyb = d.hf > 0 ? 1 : 0;
  q.lstm = d.lstm ? 1 : 0;
  int* ip = reinterpret_cast<int*>(base + bl.state);
  q.hptr = reinterpret_cast<const float**>(ip); ip += 2;  // (256-byte aligned: first in the region)
  q.frames = d.flen;
  q.maxlens = ip; ip += B;
  q.nact = ip; ip += B;
  q.nfin = ip; ip += B;
  q.done = ip; ip += B;
  q.yprev = ip; ip += R;
  q.hist = ip; ip += 2L * R * L1;
  q.hlen = ip; ip += 2 * R;
  q.fseq = ip; ip += (long)R * L1;
  q.flen = ip; ip += R;
  q.lab2 = ip;
  float* fp = reinterpret_cast<float*>(base + bl.fstate);
  q.pbeam = fp; fp += R;
  q.s = fp; fp += 2L * R * S;
  q.fscore = fp; fp += R;
  q.alpha = fp; fp += v.d2.vh_rows > 0 && d.hf == 0 ? 0 : 2L * R * d.L;
  q.mem = fp; fp += d.lstm ? 2L * R * S : 0;
  q.mlp_in = fp;
  v.k.P = P;
  v.k.h = v.hrep;
  v.k.labels = q.lab2;
  v.k.logp = nullptr;
  v.k.t = 1;
  v.gws = attn_gemm_ws(v.d2, base + bl.scratch);
  return 0;
}

int attn_beam_init(hipStream_t st, const AttnDims& d, const float* h, const AttnParams& P, int eos, int K, int maxlen,
                   void* ws, size_t ws_bytes) {
  BeamView v;
  S2S_TRY(beam_view(d, P, eos, K, maxlen, ws, ws_bytes, v));
  const int B = d.B, R = B * K, L = d.L;
  const bool shared = v.d2.vh_rows > 0;
  decide("beam.attn.path", shared ? 1 : 0);  // 1: Vh / h once per utterance (beam_f2_shared), 0: per hypothesis row
  decide("beam.layout.overlay", v.overlay ? 1 : 0);
  if (shared) {
    // Vh once per utterance (Attention.lua:356-357: vh = Vh:forward(annotations)); the steps read the caller's h
    S2S_TRY(gemm1(st, false, true, B * L, d.Sc, d.A, 1.f, h, d.A, P.V, d.A, 0.f, v.k.Vh, d.Sc, nullptr, v.gws));
  } else {
    // annotations and Vh once per hypothesis row
    hipLaunchKernelGGL(beam_rep_h, dim3(64, B), dim3(256), 0, st, h, v.hrep, K, (long)L * d.A);
    S2S_TRY(gemm1(st, false, true, R * L, d.Sc, d.A, 1.f, v.hrep, d.A, P.V, d.A, 0.f, v.k.Vh, d.Sc, nullptr, v.gws));
  }
  hipLaunchKernelGGL(beam_init, dim3(64), dim3(256), 0, st, v.q, h);
  if (d.hf > 0) hipLaunchKernelGGL(dec_hyb_fold, dim3((d.Sc + 255) / 256), dim3(256), 0, st, v.k);
  if (d.lstm) hipLaunchKernelGGL(dec_lstm_pack, dim3(256), dim3(256), 0, st, v.k);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

// per-utterance limits (device, B) in place of maxlen for every utterance, between init and the first step
// (timit.lua:400 searches each utterance to its own frame count)
int attn_beam_set_maxlens(hipStream_t st, const AttnDims& d, int K, int maxlen, const int* maxlens, void* ws) {
  BeamView v;
  AttnParams P{};
  S2S_TRY(beam_view(d, P, 0, K, maxlen, ws, beam_layout(d, K, maxlen).total, v));
  S2S_REQUIRE(maxlens, "beam search: null maxseqlengths");
  hipLaunchKernelGGL(beam_set_maxlens, dim3((d.B + 255) / 256), dim3(256), 0, st, v.q, maxlens);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

// one decoder_base forward of every active hypothesis (Attention.lua:386-399); with the fused decoder_mlp
// through the log-probabilities, with an external one up to its input rows (beam mlp_in)
int attn_beam_step(hipStream_t st, const AttnDims& d, const AttnParams& P, int K, int maxlen, int count, void* ws,
                   size_t ws_bytes) {
  BeamView v;
  S2S_TRY(beam_view(d, P, 0, K, maxlen, ws, ws_bytes, v));
  AttnK& k = v.k;
  const int R = d.B * K, S = d.S, rows = 2 * R;
  hipLaunchKernelGGL(beam_prep, dim3(64), dim3(256), 0, st, k, v.q, count & 1);
  const bool shared = v.d2.vh_rows > 0;
  decide("beam.attn.path", shared ? 1 : 0);
  decide("beam.layout.overlay", v.overlay ? 1 : 0);  // the step's post-combine buffers live inside PC (carve)
  // 16 waves, one frame each: a wave scores its frame for up to K hypotheses in turn, so the serial chain per
  // launch is K frames' worth where dec_f2_attn<8>'s is 2 (the wave count does not change a bit of the results)
  const auto f2 = d.hf > 0 ? beam_f2_shared<16, true> : beam_f2_shared<16, false>;
  // the training loop's step launches (attn.hip), unfolded: a search has no teacher-forced rows to fold KD from
  launch_fwd_step(st, k, R, false, d.lstm, nullptr, nullptr, [&] {
    if (shared) hipLaunchKernelGGL(f2, dim3(k.NCH, d.B), dim3(1024), 0, st, k, v.q);
    else hipLaunchKernelGGL(dec_f2_attn<8>, dim3(k.NCH, R), dim3(512), 0, st, k);
  });
  if (d.ext) {
    hipLaunchKernelGGL(beam_mlp_rows, dim3(256), dim3(256), 0, st, k, v.q);
  } else {
    S2S_TRY(gemm1(st, false, true, rows, d.M * d.K, S + d.A, 1.f, k.VV, S + d.A, P.Wm, S + d.A, 0.f, k.U,
                  (long)d.M * d.K, P.bm, v.gws));
    hipLaunchKernelGGL(dec_mlp_head, dim3((rows + 3) / 4), dim3(256), 4 * d.M * sizeof(float), st, k, rows);
  }
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

const float* attn_beam_mlp_input(const AttnDims& d, int K, int maxlen, void* ws) {
  BeamView v;
  AttnParams P{};
  if (beam_view(d, P, 0, K, maxlen, ws, beam_layout(d, K, maxlen).total, v) != 0) return nullptr;
  return v.q.mlp_in;
}

// topk + bookkeeping of the step (Attention.lua:400-430); logp_ext: (R, O) log-probabilities of an external
// decoder_mlp (null with the fused one)
int attn_beam_advance(hipStream_t st, const AttnDims& d, int eos, int K, int maxlen, int count, const float* logp_ext,
                      void* ws, size_t ws_bytes) {
  BeamView v;
  AttnParams P{};
  S2S_TRY(beam_view(d, P, eos, K, maxlen, ws, ws_bytes, v));
  S2S_REQUIRE(!d.ext || logp_ext, "beam search: an external decoder_mlp needs the step's log-probabilities");
  if (logp_ext) hipLaunchKernelGGL(beam_put_logp, dim3(256), dim3(256), 0, st, v.k, v.q, logp_ext);
  hipLaunchKernelGGL(beam_update, dim3(d.B), dim3(256), 0, st, v.k, v.q, count);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

int attn_beam_done(hipStream_t st, const AttnDims& d, int K, int maxlen, void* ws, int* all_done) {
  BeamView v;
  AttnParams P{};
  S2S_TRY(beam_view(d, P, 0, K, maxlen, ws, beam_layout(d, K, maxlen).total, v));
  std::vector<int> done(d.B);
  S2S_CHECK_HIP(hipMemcpyAsync(done.data(), v.q.done, sizeof(int) * d.B, hipMemcpyDeviceToHost, st));
  S2S_CHECK_HIP(hipStreamSynchronize(st));
  bool all = true;
  for (int x : done) all = all && x;
  *all_done = all ? 1 : 0;
  return 0;
}

int attn_beam_finish(hipStream_t st, const AttnDims& d, int K, int maxlen, void* ws, int* out, int ldo, int* out_len,
                     float* out_score) {
  BeamView v;
  AttnParams P{};
  S2S_TRY(beam_view(d, P, 0, K, maxlen, ws, beam_layout(d, K, maxlen).total, v));
  S2S_REQUIRE(ldo >= maxlen + 1, "beam search: ldo < maxseqlength + 1");
  hipLaunchKernelGGL(beam_final, dim3(d.B), dim3(256), 0, st, v.q, out, ldo, out_len, out_score);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

// diagnostic: every finished hypothesis of the search, the reference's y_finished / p_finished
// (Attention.lua:375-376), copied device to device in stream order; entries at or beyond nfin[b] are unspecified
int attn_beam_finished(hipStream_t st, const AttnDims& d, int K, int maxlen, void* ws, int* nfin, int* flen,
                       float* fscore, int* fseq) {
  BeamView v;
  AttnParams P{};
  S2S_TRY(beam_view(d, P, 0, K, maxlen, ws, beam_layout(d, K, maxlen).total, v));
  const size_t R = (size_t)d.B * K, L1 = (size_t)maxlen + 1;
  S2S_CHECK_HIP(hipMemcpyAsync(nfin, v.q.nfin, sizeof(int) * d.B, hipMemcpyDeviceToDevice, st));
  S2S_CHECK_HIP(hipMemcpyAsync(flen, v.q.flen, sizeof(int) * R, hipMemcpyDeviceToDevice, st));
  S2S_CHECK_HIP(hipMemcpyAsync(fscore, v.q.fscore, sizeof(float) * R, hipMemcpyDeviceToDevice, st));
  S2S_CHECK_HIP(hipMemcpyAsync(fseq, v.q.fseq, sizeof(int) * R * L1, hipMemcpyDeviceToDevice, st));
  return 0;
}

int attn_beam_search(hipStream_t st, const AttnDims& d, const float* h, const AttnParams& P, int eos, int K,
                     int maxlen, const int* maxlens, int* out, int ldo, int* out_len, float* out_score, void* ws,
                     size_t ws_bytes) {
  S2S_REQUIRE(!d.ext, "beam search: an external decoder_mlp runs through the stepwise calls");
  S2S_REQUIRE(ldo >= maxlen + 1, "beam search: ldo < maxseqlength + 1");
  S2S_TRY(attn_beam_init(st, d, h, P, eos, K, maxlen, ws, ws_bytes));
  if (maxlens) S2S_TRY(attn_beam_set_maxlens(st, d, K, maxlen, maxlens, ws));
  for (int count = 0; count <= maxlen; ++count) {
    S2S_TRY(attn_beam_step(st, d, P, K, maxlen, count, ws, ws_bytes));
    S2S_TRY(attn_beam_advance(st, d, eos, K, maxlen, count, nullptr, ws, ws_bytes));
    if ((count & 3) == 3 || count == maxlen) {  // stop once every utterance has K finished hypotheses
      int all = 0;
      S2S_TRY(attn_beam_done(st, d, K, maxlen, ws, &all));
      if (all) break;
    }
  }
  return attn_beam_finish(st, d, K, maxlen, ws, out, ldo, out_len, out_score);
}

int edit_distance(hipStream_t st, int n, const int* a, const int* alen, int lda, const int* b, const int* blen,
                  int ldb, int* out) {
  S2S_REQUIRE(n >= 0 && lda >= 0 && ldb >= 0 && lda < 16384, "edit distance: bad sizes");
  if (n == 0) return 0;
  hipLaunchKernelGGL(edit_distance_kernel, dim3(n), dim3(64), sizeof(int) * (lda + 1), st, n, a, alen, lda, b, blen,
                     ldb, out);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

int nll_seed(hipStream_t st, int B, int T, int O, const float* logp, const int* labels, int normalize, float* nll,
             float* dlogp, const int* tlen) {
  hipLaunchKernelGGL(nll_seed_kernel, dim3(B), dim3(256), 0, st, B, T, O, logp, labels, normalize, nll, dlogp, tlen);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

