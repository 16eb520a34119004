// The per-step decoder kernels (F1-F7, K2-K8, their folds) and the small utility kernels; included by attn.hip.
__device__ __forceinline__ int brow(int b0, int lane, int B) { return min(b0 + (lane & 15), B - 1); }
// frames / labels of utterance b in a variable-length batch
__device__ __forceinline__ int frames_of(const AttnK& k, int b) { return k.flen ? k.flen[b] : k.L; }
__device__ __forceinline__ int labels_of(const AttnK& k, int b) { return k.tlen ? k.tlen[b] : k.T; }

// ------------------------------------------------------------------ forward step kernels

// ---- hybrid location-aware attention (Attention.lua:75-98), per-step path only
// F = TemporalConvolution(1, nF, kW)(pad(alpha_{t-1})) with bias, UF = TCZB(nF, Sc, 1)(F): both are
// linear in alpha_{t-1}, so UF_{l,j} = HCU_j + sum_i HG_{j,i} alpha_{t-1}[l + i - pad_left] with
// HG = U W (Sc x kW) and HCU = U b, folded once per call (dec_hyb_fold).
__device__ __forceinline__ int hyb_pad_left(int kw) { return kw % 2 ? (kw - 1) / 2 : kw / 2; }

__global__ void dec_hyb_fold(AttnK k) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k.Sc) return;
  const int nf = k.hf, kw = k.hk;
  const float* u = k.P.hybU + (long)j * nf;
  for (int i = 0; i < kw; ++i) {
    float s = 0.f;
    for (int f = 0; f < nf; ++f) s += u[f] * k.P.hybW[f * kw + i];
    k.HGT[(long)i * k.Sc + j] = s;
  }
  float c = 0.f;
  for (int f = 0; f < nf; ++f) c += u[f] * k.P.hybb[f];
  k.HCU[j] = c;
}

// alpha_{t-1} of frames ch*LC - pad_left .. ch*LC + LC - 1 + (kW - 1 - pad_left) into apl (0 outside [0, L) and
// at t = 0): apl[lloc + i] is the tap-i input of chunk frame lloc.  All threads call it; ends on a barrier.
__device__ __forceinline__ void hyb_stage_alpha(const AttnK& k, const float* ap, int ch, float* apl) {
  const int pl = hyb_pad_left(k.hk), n = LC + k.hk - 1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int m = ch * LC + i - pl;
    apl[i] = (ap && m >= 0 && m < k.L) ? ap[m] : 0.f;
  }
  __syncthreads();
}
// UF of chunk frame lloc for the 4 score columns of float4 c4 (UF_{l,j} = HCU_j + sum_i HG_{j,i} apl[lloc + i]);
// apl = the staged alpha_{t-1} halo, hg = the taps HGT ([kW][Sc], global or staged in LDS)
__device__ __forceinline__ float4 hyb_uf4_lds(const AttnK& k, int c4, const float* apl, const float* hg, int lloc) {
  float4 u = reinterpret_cast<const float4*>(k.HCU)[c4];
  for (int i = 0; i < k.hk; ++i) {
    const float a = apl[lloc + i];
    const float4 g = reinterpret_cast<const float4*>(hg + (long)i * k.Sc)[c4];
    u.x += g.x * a; u.y += g.y * a; u.z += g.z * a; u.w += g.w * a;
  }
  return u;
}

// d alpha_t[l] from the hybrid features of step t + 1: sum_i q_{t+1}[l - i + pad_left][i]
__device__ __forceinline__ float hyb_carry(const AttnK& k, int b, int l) {
  if (k.t + 1 >= k.T) return 0.f;
  const int kw = k.hk, pl = hyb_pad_left(kw);
  const float* q = k.QA + ((long)((k.t + 1) & 1) * k.B + b) * k.L * kw;
  float s = 0.f;
  for (int i = 0; i < kw; ++i) {
    const int lp = l - i + pl;
    if (lp >= 0 && lp < k.L) s += q[(long)lp * kw + i];
  }
  return s;
}

// weight gradients of the hybrid features from DGT = sum dG^T (kW x Sc) and DCU = sum dws (Sc):
// G = U W, cu = U b  ->  dU = dG W^T + dcu b^T, dW = U^T dG, db = U^T dcu
// one wave per output element: the dW / db sums run over Sc across the lanes (a thread-serial loop over Sc put ~160
// dependent L2 loads behind each of those outputs: 33 us at the conv + BiLSTM model's Sc = 160)
__global__ __launch_bounds__(256) void dec_hyb_wgrad(AttnK k, AttnGrads G, float scale) {
  const int nf = k.hf, kw = k.hk, Sc = k.Sc, lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx < Sc * nf) {
    const int j = idx / nf, f = idx % nf;
    if (lane == 0) {
      float v = 0.f;
      for (int i = 0; i < kw; ++i) v += k.DGT[(long)i * Sc + j] * k.P.hybW[f * kw + i];
      v += k.DCU[j] * k.P.hybb[f];
      G.hybU[idx] += scale * v;
    }
  } else if (idx < Sc * nf + nf * kw) {
    const int r = idx - Sc * nf, f = r / kw, i = r % kw;
    float v = 0.f;
    for (int j = lane; j < Sc; j += 64) v += k.P.hybU[(long)j * nf + f] * k.DGT[(long)i * Sc + j];
    v = wave_sum(v);
    if (lane == 0) G.hybW[r] += scale * v;
  } else if (idx < Sc * nf + nf * kw + nf) {
    const int f = idx - Sc * nf - nf * kw;
    float v = 0.f;
    for (int j = lane; j < Sc; j += 64) v += k.P.hybU[(long)j * nf + f] * k.DCU[j];
    v = wave_sum(v);
    if (lane == 0) G.hybb[f] += scale * v;
  }
}

// F1: ws[b] = Ws s_{t-1}[b] + bs  (N = Sc, K = S)
__global__ __launch_bounds__(256) void dec_f1_ws(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  if (t > 0)
    acc = skinny_wave(k.HX + ((long)brow(b0, lane, k.B) * k.T + t) * 2 * S, k.P.Ws + (long)(n0 + (lane & 15)) * S,
                      S, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b < k.B) k.WS[((long)b * k.T + t) * k.Sc + n] = s + k.P.bs[n];
}

// F2: scores + chunk-local softmax stats + partial context.  grid (NCH, B)
// WV waves per workgroup (LC / WV frames each): every frame's score is one wave's, so the wave count does not
// change a bit of the results; the training loop runs 8 (half the serial frame chain of 4 x 4)
template <int WV>
__global__ __launch_bounds__(64 * WV) void dec_f2_attn(AttnK k) {
  constexpr int FPW = LC / WV, NT = 64 * WV;
  __shared__ float sc[LC];
  __shared__ float pw[LC];
  __shared__ float apl[LC + kMaxHybK];  // hybrid: alpha_{t-1} halo of the chunk (hyb_stage_alpha)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ch = blockIdx.x, b = blockIdx.y, t = k.t;
  const int L = k.L, Sc = k.Sc, A = k.A;
  const float* ws = k.WS + ((long)b * k.T + t) * Sc;
  const float* we = k.P.we;
  const float* ap = (k.hf > 0 && t > 0) ? k.ALPHA + ((long)b * k.T + t - 1) * L : nullptr;  // alpha_{t-1}
  if (k.hf > 0) hyb_stage_alpha(k, ap, ch, apl);
  const int Lb = frames_of(k, b);
  for (int i = 0; i < FPW; ++i) {
    const int li = wave * FPW + i, l = ch * LC + li;
    float part = 0.f;
    if (l < Lb) {
      const float* vh = k.Vh + ((long)b * L + l) * Sc;
      for (int c4 = lane; c4 < Sc / 4; c4 += 64) {
        float4 v = reinterpret_cast<const float4*>(vh)[c4];
        const float4 w = reinterpret_cast<const float4*>(ws)[c4];
        const float4 e = reinterpret_cast<const float4*>(we)[c4];
        float4 z = make_float4(w.x + v.x, w.y + v.y, w.z + v.z, w.w + v.w);
        if (k.hf > 0) {  // Z = Ws + Vh + UF (Attention.lua:95)
          const float4 u = hyb_uf4_lds(k, c4, apl, k.HGT, li);
          z.x += u.x; z.y += u.y; z.z += u.z; z.w += u.w;
        }
        part += e.x * tanhf(z.x) + e.y * tanhf(z.y) + e.z * tanhf(z.z) + e.w * tanhf(z.w);
      }
    }
    part = wave_sum(part);
    if (lane == 0) sc[li] = l < Lb ? part : -INFINITY;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int i = 0; i < LC; ++i) m = fmaxf(m, sc[i]);
  if (tid < LC) {
    const int l = ch * LC + tid;
    const float p = l < Lb ? expf(sc[tid] - m) : 0.f;
    pw[tid] = p;
    if (l < L) k.E[((long)b * k.T + t) * L + l] = sc[tid];
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < LC; ++i) s += pw[i];
    k.PM[b * k.NCH + ch] = m;
    k.PL[b * k.NCH + ch] = s;
  }
  float* pc = k.PC + ((long)b * k.NCH + ch) * A;
  const int lend = min(LC, L - ch * LC);
  for (int a4 = tid; a4 < A / 4; a4 += NT) {
    // every frame's row load in flight before the first add; the sum runs in frame order (as before)
    float4 hv[LC];
#pragma unroll
    for (int i = 0; i < LC; ++i)
      hv[i] = i < lend ? reinterpret_cast<const float4*>(k.h + ((long)b * L + ch * LC + i) * A)[a4]
                       : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < LC; ++i) {
      if (i < lend) {
        const float p = pw[i];
        acc.x += p * hv[i].x; acc.y += p * hv[i].y; acc.z += p * hv[i].z; acc.w += p * hv[i].w;
      }
    }
    reinterpret_cast<float4*>(pc)[a4] = acc;
  }
}

// F3: combine chunks (grid B): lse, alpha, c, MonoAlign indicator
__global__ __launch_bounds__(256) void dec_f3_combine(AttnK k) {
  __shared__ float wj[64];
  __shared__ float red[4];
  __shared__ float stat[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, t = k.t;
  const int L = k.L, A = k.A, S = k.S, NCH = k.NCH;
  const long row = (long)b * k.T + t;
  if (tid == 0) {
    float m = -INFINITY;
    for (int j = 0; j < NCH; ++j) m = fmaxf(m, k.PM[b * NCH + j]);
    float den = 0.f;
    for (int j = 0; j < NCH; ++j) {
      const float w = expf(k.PM[b * NCH + j] - m);
      if (j < 64) wj[j] = w;
      den += w * k.PL[b * NCH + j];
    }
    stat[0] = m;
    stat[1] = den;
    k.LSE[row] = m + logf(den);
  }
  __syncthreads();
  const float m = stat[0], inv = 1.0f / stat[1];
  // context c = sum_j w_j pc_j / den  -> C and the MLP input VV[:, S:]
  for (int a = tid; a < A; a += 256) {
    float acc = 0.f;
    for (int j = 0; j < NCH; ++j) {
      const float w = j < 64 ? wj[j] : expf(k.PM[b * NCH + j] - m);
      acc += w * k.PC[((long)b * NCH + j) * A + a];
    }
    const float c = acc * inv;
    k.C[row * A + a] = c;
    k.VV[row * (S + A) + S + a] = c;
  }
  // alpha_l = exp(e_l - lse) and sum_l (L - l)(alpha_l - alpha_prev_l)   (MonotonicAlignment.lua:27-35)
  const float lse = m + logf(stat[1]);
  const int Lb = frames_of(k, b);
  float diff = 0.f;
  for (int l = tid; l < L; l += 256) {
    const float a = expf(k.E[row * L + l] - lse);  // 0 on padding frames (E = -inf)
    k.ALPHA[row * L + l] = a;
    const float ap = t > 0 ? k.ALPHA[(row - 1) * L + l] : 0.f;  // alpha_{t-1} (written by step t-1)
    diff += (float)(Lb - l) * (a - ap);
  }
  diff = wave_sum(diff);
  if (lane == 0) red[wave] = diff;
  __syncthreads();
  if (tid == 0) {
    const float d = ((red[0] + red[1]) + red[2]) + red[3];
    const float pen = k.penalty * fmaxf(d, 0.f);
    k.IND[row] = (pen > 0.f && t < labels_of(k, b)) ? 1.f : 0.f;
  }
}

// F4: c_in = Wc c + bc (N = S, K = A); y_in = Wy[:, y_{t-1}] + by   -> CY = [c_in | y_in]
__global__ __launch_bounds__(256) void dec_f4_cin(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S, A = k.A;
  floatx4 acc = skinny_wave(k.C + ((long)brow(b0, lane, k.B) * k.T + t) * A, k.P.Wc + (long)(n0 + (lane & 15)) * A,
                            A, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  const long row = (long)b * k.T + t;
  k.CY[row * 2 * S + n] = s + k.P.bc[n];
  float yin = k.P.by[n];
  // y_{t-1} one-hot (teacher forcing, RNNAttention.lua:172-176); a negative label = zeros_y (beam search's
  // first step, Attention.lua:359)
  if (t > 0 && k.labels[(long)b * k.T + t - 1] >= 0) yin += k.P.Wy[(long)n * k.O + k.labels[(long)b * k.T + t - 1]];
  k.CY[row * 2 * S + S + n] = yin;
}

// F5: d = Wd [c_in; y_in] + bd (N = S, K = 2S) -> HX[:, S:] and RHX[:, S:]
__global__ __launch_bounds__(256) void dec_f5_d(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave(k.CY + ((long)brow(b0, lane, k.B) * k.T + t) * 2 * S,
                            k.P.Wd + (long)(n0 + (lane & 15)) * 2 * S, 2 * S, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  const long row = (long)b * k.T + t;
  const float d = s + k.P.bd[n];
  k.HX[row * 2 * S + S + n] = d;
  k.RHX[row * 2 * S + S + n] = d;
}

// ---- folded F4 + F5 of the per-step path (LSTM decoder / hybrid attention: the shapes the XCD-local kernels do
// not serve).  d = Wd [Wc c + bc; y_in] + bd = WDC c + KD with WDC = Wd_c Wc (S x A) and KD = Wd_y y_in + Wd_c bc
// + bd per row (teacher-forced y_in), both formed before the loop -- one launch per step instead of two.
// y_in rows of every step: CY[:, S:] = by + Wy[:, y_{t-1}] (zeros_y at t = 0 or a negative label)
__global__ void dec_fold_yin(AttnK k) {
  const int S = k.S;
  const long n = (long)k.B * k.T * S;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / S;
    const int j = (int)(i - row * S), t = (int)(row % k.T);
    float v = k.P.by[j];
    if (t > 0 && k.labels[row - 1] >= 0) v += k.P.Wy[(long)j * k.O + k.labels[row - 1]];
    k.CY[row * 2 * S + S + j] = v;
  }
}
// F45: d = WDC c_t + KD_t (N = S, K = A) -> HX[:, S:] and RHX[:, S:]
__global__ __launch_bounds__(512) void dec_f45_fold(AttnK k, const float* __restrict__ wdc, const float* __restrict__ kd) {
  __shared__ SkinnyRed8 red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S, A = k.A;
  floatx4 acc = skinny_wave8(k.C + ((long)brow(b0, lane, k.B) * k.T + t) * A, wdc + (long)(n0 + (lane & 15)) * A, A,
                            wave, lane);
  const float s = skinny_reduce8(red, acc, wave, lane, tid);
  if (tid >= 256) return;
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  const long row = (long)b * k.T + t;
  const float d = s + kd[row * S + n];
  k.HX[row * 2 * S + S + n] = d;
  k.RHX[row * 2 * S + S + n] = d;
}

// F6: [z|r] = sig(W{z,r} [s_{t-1}; d])  (N = 2S, K = 2S)
__global__ __launch_bounds__(256) void dec_f6_gru1(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  const float* W = n0 < S ? k.P.Wz + (long)n0 * 2 * S : k.P.Wr + (long)(n0 - S) * 2 * S;
  floatx4 acc = skinny_wave(k.HX + ((long)brow(b0, lane, k.B) * k.T + t) * 2 * S, W + (long)(lane & 15) * 2 * S,
                            2 * S, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  const long row = (long)b * k.T + t;
  const float g = sigmoidf_(s);
  if (n < S) {
    k.GSV[row * 3 * S + n] = g;
  } else {
    const int j = n - S;
    k.GSV[row * 3 * S + S + j] = g;
    k.RHX[row * 2 * S + j] = g * k.HX[row * 2 * S + j];
  }
}

// F7: hh = tanh(Wh [r*s; d]); s_t = (1-z) s_{t-1} + z hh  (N = S, K = 2S)
__global__ __launch_bounds__(256) void dec_f7_gru2(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave(k.RHX + ((long)brow(b0, lane, k.B) * k.T + t) * 2 * S,
                            k.P.Wh + (long)(n0 + (lane & 15)) * 2 * S, 2 * S, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  const long row = (long)b * k.T + t;
  const float hh = tanhf(s);
  const float z = k.GSV[row * 3 * S + n], sp = k.HX[row * 2 * S + n];
  k.GSV[row * 3 * S + 2 * S + n] = hh;
  const float snew = (-z + 1.0f) * sp + z * hh;
  k.VV[row * (S + k.A) + n] = snew;
  if (t + 1 < k.T) k.HX[(row + 1) * 2 * S + n] = snew;
}

// ---- decoder LSTM (LSTM.lua:16-58 as decoder_recurrent, timit/timit.lua:137): s = h, mem = c
// LW rows interleave the four gates of each unit: row 4 u + q = [Wqh[u] | Wqx[u]] (q = i, f, g, o) against HX rows
// [s_{t-1} | d]; LB[4 u + q] = bqx + bqh.  (GT, the backward's LW^T, keeps the gate-major column order q S + u of
// the gate gradients: dec_lstm_gt.)
__global__ void dec_lstm_pack(AttnK k) {
  const int S = k.S;
  const long n = 4L * S * 2 * S;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / (2 * S)), c = (int)(i - (long)r * 2 * S), u = r >> 2, q = r & 3;
    k.LW[i] = c < S ? k.P.lstm[4 * q + 2][(long)u * S + c] : k.P.lstm[4 * q][(long)u * S + c - S];
    if (c == 0) k.LB[r] = k.P.lstm[4 * q + 1][u] + k.P.lstm[4 * q + 3][u];
  }
}
// GT (2S, 4S) = LW^T with the gate-major column order of the gate gradients: GT[n][q S + u] = LW[4 u + q][n]
__global__ void dec_lstm_gt(AttnK k) {
  const int S = k.S;
  const long n = 2L * S * 4 * S;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i / (4 * S)), j = (int)(i - (long)c * 4 * S), q = j / S, u = j - q * S;
    k.GT[i] = k.LW[(long)(4 * u + q) * 2 * S + c];
  }
}

// F6 + F7 (LSTM), one launch per step: the block's 16 output rows are the four gates of four units (LW's
// interleaved rows), gate = act(LW[4u+q] . [s_{t-1}; d] + LB) (N = 4S, K = 2S; act = sigmoid, g: tanh), then
// the unit's four gates meet in four adjacent lanes and the lane of gate i updates the cell: c = f c_{t-1} + i g,
// s = o tanh(c).  (The cell update used to be its own launch per decoder step.)
__global__ __launch_bounds__(512) void dec_f6_lstm(AttnK k) {
  __shared__ SkinnyRed8 red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave8(k.HX + ((long)brow(b0, lane, k.B) * k.T + t) * 2 * S,
                            k.LW + (long)(n0 + (lane & 15)) * 2 * S, 2 * S, wave, lane);
  const float s = skinny_reduce8(red, acc, wave, lane, tid);
  if (tid >= 256) return;
  const int b = b0 + (tid >> 4), r = n0 + (tid & 15), u = r >> 2, q = r & 3;
  if (b >= k.B) return;  // (uniform over each group of four lanes: one row)
  const long row = (long)b * k.T + t;
  const float x = s + k.LB[r];
  const float gv = q == 2 ? tanhf(x) : sigmoidf_(x);
  k.GSV[row * 4 * S + q * S + u] = gv;
  const int l0 = lane & ~3;
  const float gi = __shfl(gv, l0, 64), gf = __shfl(gv, l0 + 1, 64), gg = __shfl(gv, l0 + 2, 64),
              go = __shfl(gv, l0 + 3, 64);
  if (q != 0) return;
  const float cp = t > 0 ? k.LC[(row - 1) * S + u] : 0.f;
  const float c = gf * cp + gi * gg;
  const float snew = go * tanhf(c);
  k.LC[row * S + u] = c;
  k.VV[row * (S + k.A) + u] = snew;
  if (t + 1 < k.T) k.HX[(row + 1) * 2 * S + u] = snew;
}

__global__ void dec_init_fwd(AttnK k) {
  // s_0 = 0 (Recurrent.lua:112 zeros_hidden)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k.B * k.S) {
    const int b = i / k.S, n = i - b * k.S;
    k.HX[((long)b * k.T) * 2 * k.S + n] = 0.f;
  }
}

// MLP head (per row b*T+t, one wave each): maxout (first max wins), Linear(M,O), LogSoftMax; with k.dlogp set (the
// seed is final before the forward, AttnDims::dlogp_early) also its backward, dec_mlp_head_bwd's per-row work with
// the same sums: do = dlogp - exp(logp) sum(dlogp), dm = Wo^T do, dU = scatter(dm, argmax).  LDS: 4 M (+ 4 O) floats
__device__ __forceinline__ void mlp_head_body(const AttnK& k, int rows, int blk) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blk * 4 + wave;
  const int M = k.M, Kw = k.K, O = k.O;
  float* mv = sm + wave * M;
  const bool live = r < rows;
  if (live) {
    const float* u = k.U + (long)r * M * Kw;
    // U[r][c] from the MLP GEMM's slabs when it left them unreduced: splitk_reduce's expression (alpha = 1)
    auto uv = [&](int c) -> float {
      if (!k.UP) return u[c];
      const long e = (long)r * M * Kw + c;
      float sum = 0.f;
      for (int s = 0; s < k.UPS; ++s) sum += k.UP[s * k.UPMN + e];
      return 1.f * sum + k.P.bm[c];
    };
    for (int j = lane; j < M; j += 64) {
      float best = uv(j * Kw);
      int bi = 0;
      for (int i = 1; i < Kw; ++i) {
        const float v = uv(j * Kw + i);
        if (v > best) { best = v; bi = i; }
      }
      mv[j] = best;
      k.MM[(long)r * M + j] = best;
      k.AM[(long)r * M + j] = bi;
    }
  }
  __syncthreads();
  if (live) {
    float mx = -INFINITY;
    for (int n = lane; n < O; n += 64) {
      float o = k.P.bo[n];
      const float* w = k.P.Wo + (long)n * M;
      for (int j = 0; j < M; ++j) o += w[j] * mv[j];
      k.LOGP[(long)r * O + n] = o;
      mx = fmaxf(mx, o);
    }
    mx = wave_max(mx);
    float se = 0.f;
    for (int n = lane; n < O; n += 64) se += expf(k.LOGP[(long)r * O + n] - mx);
    se = wave_sum(se);
    const float lz = mx + logf(se);
    for (int n = lane; n < O; n += 64) {
      const float v = k.LOGP[(long)r * O + n] - lz;
      k.LOGP[(long)r * O + n] = v;
      if (k.logp) k.logp[(long)r * O + n] = v;
    }
  }
  if (!k.dlogp) return;
  float* dov = sm + 4 * M + wave * O;
  float sd = 0.f;
  if (live)
    for (int n = lane; n < O; n += 64) sd += k.dlogp[(long)r * O + n];
  sd = wave_sum(sd);
  if (live)
    for (int n = lane; n < O; n += 64) {
      const float v = k.dlogp[(long)r * O + n] - expf(k.LOGP[(long)r * O + n]) * sd;
      dov[n] = v;
      k.DO[(long)r * O + n] = v;
    }
  __syncthreads();
  if (!live) return;
  float* du = k.DU + (long)r * M * Kw;
  for (int j = lane; j < M; j += 64) {
    float dm = 0.f;
    for (int n = 0; n < O; ++n) dm += k.P.Wo[(long)n * M + j] * dov[n];
    const int am = k.AM[(long)r * M + j];
    for (int i = 0; i < Kw; ++i) du[j * Kw + i] = i == am ? dm : 0.f;
  }
}
__global__ __launch_bounds__(256) void dec_mlp_head(AttnK k, int rows) { mlp_head_body(k, rows, blockIdx.x); }

// ------------------------------------------------------------------ backward kernels

// per row: do = dlogp - exp(logp) sum(dlogp) (LogSoftMax bwd); dm = Wo^T do; du = scatter(dm, argmax)
__global__ __launch_bounds__(256) void dec_mlp_head_bwd(AttnK k, int rows) {
  extern __shared__ float sm[];  // 4 * O
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x * 4 + wave;
  const int M = k.M, Kw = k.K, O = k.O;
  float* dov = sm + wave * O;
  float sd = 0.f;
  if (r < rows)
    for (int n = lane; n < O; n += 64) sd += k.dlogp[(long)r * O + n];
  sd = wave_sum(sd);
  if (r < rows)
    for (int n = lane; n < O; n += 64) {
      const float v = k.dlogp[(long)r * O + n] - expf(k.LOGP[(long)r * O + n]) * sd;
      dov[n] = v;
      k.DO[(long)r * O + n] = v;
    }
  __syncthreads();
  if (r >= rows) return;
  float* du = k.DU + (long)r * M * Kw;
  for (int j = lane; j < M; j += 64) {
    float dm = 0.f;
    for (int n = 0; n < O; ++n) dm += k.P.Wo[(long)n * M + j] * dov[n];
    const int am = k.AM[(long)r * M + j];
    for (int i = 0; i < Kw; ++i) du[j * Kw + i] = i == am ? dm : 0.f;
  }
}

__device__ __forceinline__ void dec_gate_grads(const AttnK& k, int b, int t, int n, float ds) {
  const int S = k.S;
  const long row = (long)b * k.T + t;
  const float z = k.GSV[row * 3 * S + n], hh = k.GSV[row * 3 * S + 2 * S + n], sp = k.HX[row * 2 * S + n];
  k.DS[b * S + n] = ds;
  k.DGA[row * 3 * S + n] = ds * (hh - sp) * (z * (1.0f - z));
  k.DGA[row * 3 * S + 2 * S + n] = (ds * z) * (1.0f - hh * hh);
}

// LSTM gate grads of step t from ds = dL/ds_t and the cell carry dcar = dL/dc_t from step t+1
// (LSTM.lua:118-136 under RNNAttention's BPTT); leaves dL/dc_{t-1} in DSP
__device__ __forceinline__ void dec_lstm_gate_grads(const AttnK& k, int b, int t, int n, float ds, float dcar) {
  const int S = k.S;
  const long row = (long)b * k.T + t;
  const float* g = k.GSV + row * 4 * S;
  const float gi = g[n], gf = g[S + n], gg = g[2 * S + n], go = g[3 * S + n];
  const float c = k.LC[row * S + n], cp = t > 0 ? k.LC[(row - 1) * S + n] : 0.f;
  const float tc = tanhf(c);
  const float dc = dcar + ds * go * (1.0f - tc * tc);
  float* dga = k.DGA + row * 4 * S;
  dga[n] = dc * gg * (gi * (1.0f - gi));
  dga[S + n] = dc * cp * (gf * (1.0f - gf));
  dga[2 * S + n] = dc * gi * (1.0f - gg * gg);
  dga[3 * S + n] = ds * tc * (go * (1.0f - go));
  k.DSP[b * S + n] = dc * gf;
}

__global__ void dec_bwd_init(AttnK k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k.B * k.S) return;
  const int b = i / k.S, n = i - b * k.S, t = k.T - 1;
  if (k.lstm) dec_lstm_gate_grads(k, b, t, n, k.DV[((long)b * k.T + t) * (k.S + k.A) + n], 0.f);
  else dec_gate_grads(k, b, t, n, k.DV[((long)b * k.T + t) * (k.S + k.A) + n]);
}

// K3 (LSTM): [ds_prev | dd] = LW^T dGA  (N = 2S, K = 4S; GT = LW^T)
__global__ __launch_bounds__(512) void dec_b3_lstm(AttnK k) {
  __shared__ SkinnyRed8 red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave8(k.DGA + ((long)brow(b0, lane, k.B) * k.T + t) * 4 * S,
                            k.GT + (long)(n0 + (lane & 15)) * 4 * S, 4 * S, wave, lane);
  const float s = skinny_reduce8(red, acc, wave, lane, tid);
  if (tid >= 256) return;
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  if (n < S) k.DSPF[b * S + n] = s;
  else k.DD[((long)b * k.T + t) * S + n - S] = s;
}

// K2: dq = Wh[:, :S]^T da_h (N = S, K = S) -> da_r, DSP = ds(1-z) + dq r
__global__ __launch_bounds__(256) void dec_b2_gru1(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave(k.DGA + ((long)brow(b0, lane, k.B) * k.T + t) * 3 * S + 2 * S,
                            k.WhT + (long)(n0 + (lane & 15)) * S, S, wave, lane);
  const float dq = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  const long row = (long)b * k.T + t;
  const float z = k.GSV[row * 3 * S + n], r = k.GSV[row * 3 * S + S + n], sp = k.HX[row * 2 * S + n];
  k.DGA[row * 3 * S + S + n] = (dq * sp) * (r * (1.0f - r));
  k.DSP[b * S + n] = k.DS[b * S + n] * (-z + 1.0f) + dq * r;
}

// K3: [ds_prev | dd] = GT [da_z; da_r; da_h]  (N = 2S, K = 3S)
__global__ __launch_bounds__(256) void dec_b3_gru2(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave(k.DGA + ((long)brow(b0, lane, k.B) * k.T + t) * 3 * S,
                            k.GT + (long)(n0 + (lane & 15)) * 3 * S, 3 * S, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  if (n < S) k.DSPF[b * S + n] = k.DSP[b * S + n] + s;
  else k.DD[((long)b * k.T + t) * S + n - S] = s;
}

// K4: [dc_in | dy_in] = Wd^T dd  (N = 2S, K = S)
__global__ __launch_bounds__(256) void dec_b4_wd(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave(k.DD + ((long)brow(b0, lane, k.B) * k.T + t) * S, k.WdT + (long)(n0 + (lane & 15)) * S,
                            S, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b < k.B) k.DCY[((long)b * k.T + t) * 2 * S + n] = s;
}

// K5: dc = dv_c + Wc^T dc_in  (N = A, K = S)
__global__ __launch_bounds__(256) void dec_b5_wc(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave(k.DCY + ((long)brow(b0, lane, k.B) * k.T + t) * 2 * S,
                            k.WcT + (long)(n0 + (lane & 15)) * S, S, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  const long row = (long)b * k.T + t;
  k.DC[row * k.A + n] = k.DV[row * (S + k.A) + S + n] + s;
}

// K45 (folded, the per-step path's LSTM / hybrid shapes): dc = dv_c + WDC^T dd (N = A, K = S; wdct = WDC^T);
// DCY = dd Wd for the weight gradients is one GEMM after the loop
__global__ __launch_bounds__(512) void dec_b45_fold(AttnK k, const float* __restrict__ wdct) {
  __shared__ SkinnyRed8 red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  floatx4 acc = skinny_wave8(k.DD + ((long)brow(b0, lane, k.B) * k.T + t) * S, wdct + (long)(n0 + (lane & 15)) * S, S,
                            wave, lane);
  const float s = skinny_reduce8(red, acc, wave, lane, tid);
  if (tid >= 256) return;
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B) return;
  const long row = (long)b * k.T + t;
  k.DC[row * k.A + n] = k.DV[row * (S + k.A) + S + n] + s;
}

// K6: fused attention backward for one 16-frame chunk.  grid (NCH, B)
//   d alpha_l = dc . h_l + carry_l + gdiff_l      (MM bwd + MonotonicAlignment.lua:44-77)
//   de_l = alpha_l (d alpha_l - sum_j alpha_j d alpha_j)   with sum = dc . c + sum alpha (carry + gdiff)
//   dZ = de_l we (1 - tanh^2);  dVh_l += dZ;  partial dws, dwe  (dh_l = sum_t alpha_{t,l} dc_t is one GEMM per
//   utterance after the loop, attn_dh_gemms: a read-modify-write of dh per frame and step cost 5.3 us of 28)
//   HYB (hybrid attention): Z includes UF; d alpha_l also gets the carry from step t+1's location
//   features (hyb_carry); q_{l,i} = sum_j dZ_lj HG_ji -> QA for step t-1; dG partials -> PDG
//   HYB keeps this chunk's dZ rows in LDS (dynamic, LC x Sc floats) and forms q and the dG partials from them
//   after the frame loop: per-lane register partials over every tap (kMaxHybK x 16 floats) spilled to scratch
//   at one wave per SIMD (37.7 us per step at the conv + BiLSTM model's B = 32, Sc = 160; tools/ab_convlstm.py)
template <bool HYB>
__global__ __launch_bounds__(HYB ? 512 : 256) void dec_b6_attn(AttnK k) {
  // HYB: 8 waves x 2 frames (the content-attention form keeps 4 x 4: it is bitwise equal to the persistent
  // kernels of attn_persist.inc, and the wave count sets the order of the cross-wave sums)
  constexpr int WV = HYB ? 8 : 4, FPW = LC / WV, NT = 64 * WV;
  __shared__ float redv[WV];
  __shared__ float pws[WV][1024];
  extern __shared__ float zl[];  // HYB: [LC][Sc] dZ rows of this chunk, then HGT [kW][Sc], then the alpha halo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ch = blockIdx.x, b = blockIdx.y, t = k.t;
  const int L = k.L, A = k.A, Sc = k.Sc, T = k.T;
  const long row = (long)b * T + t;
  const float* dc = k.DC + row * A;
  const float* c = k.C + row * A;
  const float* alpha = k.ALPHA + row * L;
  const float lam = k.penalty;
  const float ind = k.IND[row], indn = t + 1 < T ? k.IND[row + 1] : 0.f;
  const int Lb = frames_of(k, b);  // MonotonicAlignment's L (alpha = 0 past it)
  // sum_j alpha_j d alpha_j
  float part = 0.f;
  for (int a = tid; a < A; a += NT) part += dc[a] * c[a];
  for (int l = tid; l < L; l += NT)
    part += alpha[l] * (HYB ? lam * (float)(Lb - l) * (ind - indn) + hyb_carry(k, b, l)
                            : lam * (float)(Lb - l) * (ind - indn));
  part = wave_sum(part);
  if (lane == 0) redv[wave] = part;
  __syncthreads();
  float ssum = redv[0];
#pragma unroll
  for (int w = 1; w < WV; ++w) ssum += redv[w];
  const float* ws = k.WS + row * Sc;
  const float* we = k.P.we;
  // Sc <= 1024 asserted on the host: each lane owns k = 4*(lane + 64 i)
  float dwsp[16], dwep[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dwsp[i] = 0.f; dwep[i] = 0.f; }
  const float* ap = (HYB && t > 0) ? k.ALPHA + (row - 1) * L : nullptr;  // alpha_{t-1}
  const int lend = min(LC, L - ch * LC);  // frames of this chunk
  float* hg = zl + (long)LC * Sc;         // HYB: the taps HGT, staged
  float* apl = hg + (long)k.hk * Sc;      // HYB: alpha_{t-1} halo of the chunk
  if (HYB) {
    for (int i = tid; i < k.hk * Sc; i += NT) hg[i] = k.HGT[i];
    hyb_stage_alpha(k, ap, ch, apl);
  }
  for (int i4 = 0; i4 < FPW; ++i4) {
    const int lloc = wave * FPW + i4, l = ch * LC + lloc;
    if (l >= L) break;
    const float* hl = k.h + ((long)b * L + l) * A;
    float dd = 0.f;
    for (int a4 = lane; a4 < A / 4; a4 += 64) {
      const float4 hv = reinterpret_cast<const float4*>(hl)[a4];
      const float4 dv = reinterpret_cast<const float4*>(dc)[a4];
      dd += hv.x * dv.x + hv.y * dv.y + hv.z * dv.z + hv.w * dv.w;
    }
    dd = wave_sum(dd);
    const float al = alpha[l];
    const float dal = HYB ? dd + (lam * (float)(Lb - l) * (ind - indn) + hyb_carry(k, b, l))
                          : dd + lam * (float)(Lb - l) * (ind - indn);
    const float de = al * (dal - ssum);
    const float* vh = k.Vh + ((long)b * L + l) * Sc;
    float* dvh = k.DVH + ((long)b * L + l) * Sc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c4 = lane + 64 * i;
      if (c4 < Sc / 4) {
        const float4 v = reinterpret_cast<const float4*>(vh)[c4];
        const float4 w = reinterpret_cast<const float4*>(ws)[c4];
        const float4 e = reinterpret_cast<const float4*>(we)[c4];
        float4 o = reinterpret_cast<float4*>(dvh)[c4];
        float4 zz = make_float4(w.x + v.x, w.y + v.y, w.z + v.z, w.w + v.w);
        if (HYB) {
          const float4 u = hyb_uf4_lds(k, c4, apl, hg, lloc);
          zz.x += u.x; zz.y += u.y; zz.z += u.z; zz.w += u.w;
        }
        const float th0 = tanhf(zz.x), th1 = tanhf(zz.y), th2 = tanhf(zz.z), th3 = tanhf(zz.w);
        const float z0 = de * e.x * (1.f - th0 * th0), z1 = de * e.y * (1.f - th1 * th1);
        const float z2 = de * e.z * (1.f - th2 * th2), z3 = de * e.w * (1.f - th3 * th3);
        if (HYB) reinterpret_cast<float4*>(zl + (long)lloc * Sc)[c4] = make_float4(z0, z1, z2, z3);
        o.x += z0; o.y += z1; o.z += z2; o.w += z3;
        reinterpret_cast<float4*>(dvh)[c4] = o;
        dwsp[4 * i] += z0; dwsp[4 * i + 1] += z1; dwsp[4 * i + 2] += z2; dwsp[4 * i + 3] += z3;
        dwep[4 * i] += de * th0; dwep[4 * i + 1] += de * th1; dwep[4 * i + 2] += de * th2; dwep[4 * i + 3] += de * th3;
      }
    }
  }
  // cross-wave sums of the per-wave partials (fixed order), dws then dwe
  float* pd = k.PDWS + ((long)b * k.NCH + ch) * Sc;
  float* pe = k.DWEACC + ((long)b * k.NCH + ch) * Sc;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c4 = lane + 64 * i;
      if (c4 < Sc / 4) {
        float* dst = &pws[wave][4 * c4];
        const float* src = pass == 0 ? &dwsp[4 * i] : &dwep[4 * i];
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
      }
    }
    __syncthreads();
    for (int kk = tid; kk < Sc; kk += NT) {
      float v = pws[0][kk];
#pragma unroll
      for (int w = 1; w < WV; ++w) v += pws[w][kk];
      if (pass == 0) pd[kk] = v; else pe[kk] += v;
    }
  }
  if (HYB) {  // (the passes above ended on a barrier after every zl store)
    const int hk = k.hk;
    // q_{l,i} = sum_j dZ_lj HG_ji for d alpha_{t-1} (read by step t-1's kernel through hyb_carry): four threads
    // per (frame, tap) pair, float4 columns c4 = r, r + 4, ... then a 4-lane butterfly (a wave reduction per
    // pair cost 6.5 us of the kernel's 28 at Sc = 160, kW = 5)
    float* qa = k.QA + ((long)(t & 1) * k.B + b) * L * hk + (long)ch * LC * hk;
    for (int p0 = 0; p0 < lend * hk; p0 += NT / 4) {
      const int p = p0 + (tid >> 2), r = tid & 3;
      float q = 0.f;
      if (p < lend * hk) {
        const int lloc = p / hk, ii = p - lloc * hk;
        const float4* z4 = reinterpret_cast<const float4*>(zl + (long)lloc * Sc);
        const float4* g4 = reinterpret_cast<const float4*>(hg + (long)ii * Sc);
        for (int c4 = r; c4 < Sc / 4; c4 += 4) {
          const float4 z = z4[c4], g = g4[c4];
          q += ((z.x * g.x + z.y * g.y) + z.z * g.z) + z.w * g.w;
        }
      }
      q += __shfl_xor(q, 1, 64);
      q += __shfl_xor(q, 2, 64);
      if (p < lend * hk && r == 0) qa[p] = q;
    }
    // dG partials of this chunk, accumulated over the steps (PDG zeroed before the loop): sum_l dZ_lj
    // alpha_{t-1}[l + i - pad_left] (no term at t = 0)
    if (ap) {
      float* pg = k.PDG + ((long)b * k.NCH + ch) * hk * Sc;
      for (int e = tid; e < hk * Sc; e += NT) {
        const int ii = e / Sc, kk = e - ii * Sc;
        float g = 0.f;
        for (int lloc = 0; lloc < lend; ++lloc) g += zl[(long)lloc * Sc + kk] * apl[lloc + ii];
        pg[e] += g;
      }
    }
  }
}

// skinny_wave over the chunk-summed dws row: operand chunk = sum_j PDWS[b][j][k..k+3] in chunk order from 0 (the
// sum dec_b7_dws formed, bitwise); `store` (the workgroups of blockIdx.x == 0) also writes the summed row to DWS
__device__ __forceinline__ float4 dws_chunk(const float* __restrict__ p, int nch, long stride, int off) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = 0; j < nch; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(p + j * stride + off);
    x.x += v.x; x.y += v.y; x.z += v.z; x.w += v.w;
  }
  return x;
}
__device__ __forceinline__ floatx4 skinny_wave_dws(const float* __restrict__ prow, int nch, float* __restrict__ dws_row,
                                                   bool store, const float* __restrict__ wrow, int K, int wave,
                                                   int lane) {
  floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int kq = 4 * (lane >> 4);
  int kc = wave * 16;
  for (; kc + 64 < K; kc += 128) {
    const float4 a0 = dws_chunk(prow, nch, K, kc + kq);
    const float4 b0 = *reinterpret_cast<const float4*>(wrow + kc + kq);
    const float4 a1 = dws_chunk(prow, nch, K, kc + 64 + kq);
    const float4 b1 = *reinterpret_cast<const float4*>(wrow + kc + 64 + kq);
    if (store) {
      *reinterpret_cast<float4*>(dws_row + kc + kq) = a0;
      *reinterpret_cast<float4*>(dws_row + kc + 64 + kq) = a1;
    }
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc1, 0, 0, 0);
  }
  for (; kc < K; kc += 64) {
    const float4 a0 = dws_chunk(prow, nch, K, kc + kq);
    const float4 b0 = *reinterpret_cast<const float4*>(wrow + kc + kq);
    if (store) *reinterpret_cast<float4*>(dws_row + kc + kq) = a0;
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc0, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc0, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc0, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc0, 0, 0, 0);
  }
  return acc0 + acc1;
}

// K7 + K8: dws_t = sum over the attention chunks' partials (-> DWS, the weight gradients' rows), ds_{t-1} = DSPF +
// Ws^T dws (N = S, K = Sc); then the gate grads of step t-1.  (The chunk sum was its own launch, dec_b7_dws: one
// launch per decoder step fewer.)
__global__ __launch_bounds__(256) void dec_b8_ws(AttnK k) {
  __shared__ SkinnyRed red;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, b0 = blockIdx.y * 16, t = k.t, S = k.S;
  const int bl = b0 + (lane & 15), br = min(bl, k.B - 1);
  floatx4 acc = skinny_wave_dws(k.PDWS + (long)br * k.NCH * k.Sc, k.NCH, k.DWS + ((long)br * k.T + t) * k.Sc,
                                blockIdx.x == 0 && bl < k.B, k.WsT + (long)(n0 + (lane & 15)) * k.Sc, k.Sc, wave, lane);
  const float s = skinny_reduce(red, acc, wave, lane, tid);
  const int b = b0 + (tid >> 4), n = n0 + (tid & 15);
  if (b >= k.B || t == 0) return;
  const float carry = k.DSPF[b * S + n] + s;
  if (k.lstm) dec_lstm_gate_grads(k, b, t - 1, n, k.DV[((long)b * k.T + t - 1) * (S + k.A) + n] + carry,
                                  k.DSP[b * S + n]);
  else dec_gate_grads(k, b, t - 1, n, k.DV[((long)b * k.T + t - 1) * (S + k.A) + n] + carry);
}

// G.lstm[4 q] (Wqx) += LDW[q S + r][S + c], G.lstm[4 q + 2] (Wqh) += LDW[q S + r][c]  (LDW: (4S, 2S) gate-major)
__global__ void lstm_dw_scatter(const float* __restrict__ ldw, int S, AttnGrads G) {
  const long n = 8L * S * S;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int h = (int)(i / (4L * S * S));  // 0: x half, 1: h half
    const long e = i - h * 4L * S * S;
    const int q = (int)(e / ((long)S * S));
    const long rc = e - (long)q * S * S;
    const int r = (int)(rc / S), c = (int)(rc - (long)r * S);
    const float v = ldw[((long)q * S + r) * 2 * S + (h == 0 ? S + c : c)];
    float* dst = G.lstm[4 * q + (h == 0 ? 0 : 2)] + rc;
    *dst = *dst + v;
  }
}

__global__ void dec_onehot_prev(AttnK k) {
  // YP[b][t] = onehot(y_{t-1}), zeros at t = 0 (RNNAttention.lua:172-176)
  const long n = (long)k.B * k.T * k.O;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / k.O;
    const int o = (int)(i - row * k.O);
    const int t = (int)(row % k.T);
    k.YP[i] = (t > 0 && k.labels[row - 1] == o) ? 1.f : 0.f;
  }
}

__global__ void fill2d_kernel(float* dst, long ldd, int rows, int cols, float v) {
  const long n = (long)rows * cols;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cols, c = i - r * cols;
    dst[r * ldd + c] = v;
  }
}

__global__ void nll_seed_kernel(int B, int T, int O, const float* logp, const int* labels, int normalize, float* nll,
                                float* dlogp, const int* tlen) {
  const int b = blockIdx.x;
  __shared__ float red[4];
  const int Tb = tlen ? tlen[b] : T;  // labels of this utterance; later steps are padding
  float s = 0.f;
  for (int i = threadIdx.x; i < T * O; i += blockDim.x) {
    const int t = i / O, o = i - t * O;
    const bool hit = t < Tb && labels[b * T + t] == o;
    if (hit && logp) s += logp[((long)b * T + t) * O + o];
    if (dlogp) dlogp[((long)b * T + t) * O + o] = hit ? -1.f : 0.f;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0 && nll) {
    float v = -(((red[0] + red[1]) + red[2]) + red[3]);
    nll[b] = normalize ? v / (float)Tb : v;
  }
}

// nn.Dropout(p) (Torch7, training mode) on the decoder MLP input [s_t; c_t]
// (timit/model_chorowski_baseline_dropout.lua:56): MASK = injected multipliers, or Bernoulli(1-p)/(1-p)
// from a counter-based hash of (seed, element) -- any launch geometry draws the same mask -- and
// VV *= MASK.  The backward multiplies dVV by the same MASK (dec_dropout_bwd).
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// one word written on the stream (graph replays read each step's dropout seed from it)
__global__ void set_u64_kernel(unsigned long long* p, unsigned long long v) { *p = v; }
__global__ void dec_dropout_fwd(AttnK k, float p, unsigned long long seed, const unsigned long long* seedp,
                                const float* inj) {
  if (seedp) seed = *seedp;
  const long n = (long)k.B * k.T * (k.S + k.A);
  const float keep = 1.0f / (1.0f - p);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float m;
    if (inj) {
      m = inj[i];
    } else {
      const unsigned long long h = mix64(seed * 0x9e3779b97f4a7c15ull + (unsigned long long)i);
      const float u = (float)(h >> 40) * (1.0f / 16777216.0f);  // [0, 1)
      m = u >= p ? keep : 0.f;
    }
    k.MASK[i] = m;
    k.VV[i] = k.VV[i] * m;
  }
}
__global__ void dec_dropout_bwd(AttnK k) {
  const long n = (long)k.B * k.T * (k.S + k.A);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    k.DV[i] = k.DV[i] * k.MASK[i];
}
