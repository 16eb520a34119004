// Weight noise and Graves-style adaptive weight noise around the flat parameter vector, on the device:
// the reference's WeightNoise.lua / AdaptiveWeightNoise.lua and the trainer code around them
// (timit/timit.lua:190-205 construction, :219-253 Sample() into `parameters`, :291-333 clip / L2 / gradient
// noise then forward + backward of the noise module, :375-379 Mode() before evaluation).
//
//   adaptive: weight = [mu ; s] (2n), s = log sigma^2.
//     Sample()           parameters = mu + exp(s)^0.5 * N(0, 1)                  (AdaptiveWeightNoise.lua:27-38)
//     updateOutput(nll)  alpha_mu = mean(mu); alpha_sigma2 = max(1e-12, mean(exp s) + sum((mu - alpha_mu)^2) / n)
//                        KL = 0.5 (n log alpha_sigma2 - sum s) + 0.5 / alpha_sigma2 sum((mu - alpha_mu)^2)
//                             + 0.5 / alpha_sigma2 sum(exp s) - n / 2;   L = lambda KL + nll          (:63-80)
//     accGradParameters  dLNds = 0.5 g^2 exp(s);  gradmu = g + lambda (mu - alpha_mu) / alpha_sigma2
//                        grads = dLNds + lambda 0.5 exp(s) / alpha_sigma2 - lambda 0.5               (:82-104)
//     (lambda <= 0: L = nll, gradmu = g, grads = dLNds)
//   fixed: weight (n).  Sample() parameters = weight + sigma * N(0, 1) (WeightNoise.lua:17-22); L = nll (:28-31);
//     gradWeight = g (:33-35, after the trainer's zeroGradParameters).
// g is the model gradient after the 1/B scaling (the step's `scale`), the global-norm clip (timit.lua:297-302),
// L2 on the SAMPLED parameters (:305-308, which also adds 0.5 weightDecay ||parameters||^2 to nll) and the
// gradient noise (:310-315) -- the rules of optim.hip, which the optimizer on `weight` then must not repeat.
//
// Deviations from the reference (DESIGN.md "Weight noise"): one draw per sample() call, not per utterance
// (identical at B = 1); the draws are the counter-based normals of noise.h keyed on (sample_seed, t_s), so every
// launch geometry and data-parallel rank draws the same sample; the column-norm constraint is the optimizer's, on
// the rows of mu.
//
// All of it is streaming work over n elements (4,356,222 for the Chorowski layout): 16-byte accesses on a body
// aligned to the array each kernel writes first, scalar head and tail (at most 3 + 3 elements), grids capped at
// 2048 workgroups like opt_adadelta's.  The other arrays may sit at another 16-byte phase (s = weight + n is 8
// bytes off mu for that n): their 16-byte accesses are declared 4-byte aligned and the compiler picks the widest
// access the target allows.  No host sync: both counters, the clip factor, the noise sigma, the skip decision
// and the KL scalars live in a device state block, so a captured graph replays them.  The reduction is a fixed
// tree -- per-thread strips, per-wave shuffles, per-block partials, one block over the partials -- in double, so
// runs are bitwise repeatable and sum((mu - alpha_mu)^2) survives a mean far from zero: it is accumulated as
// sum d^2 - (sum d)^2 / n on d = mu - mu[0] (the shifted one-pass form; in fp32 without the shift alpha_sigma2
// is off by 1 % at mean 3, std 0.01).
#include "noise.h"
#include "s2s_common.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace s2s {

namespace {

constexpr int kRedBlocks = 512;
constexpr int kSums = 6;  // sum g^2, sum p^2, sum d, sum d^2 (d = mu - mu[0]), sum exp(s), sum s

// s2s_wnoise_state_bytes of device memory.  The two counters come first so a host can checkpoint them by
// copying the first 8 bytes (include/s2s_hip.h documents that).
struct WnState {
  unsigned t_sample;    // samples drawn: sample() increments it, then keys its draw on it
  unsigned t_gradnoise; // gradnoise.t (timit.lua:312): backward() increments it when gradnoise_eta != 0
  float clip;           // maxnorm / ||g|| or 1
  float gn_sigma;       // sqrt(eta / (1 + t)^gamma)
  float skip;           // nonzero: this backward is skipped (status words or skip_flag set)
  float kl_mu;          // lambda / alpha_sigma2            (0 when lambda <= 0)
  float kl_s;           // lambda * 0.5 / alpha_sigma2
  float pad0;
  double alpha_mu;
  double pad1[27];
  double partial[kSums][kRedBlocks];
};
static_assert(offsetof(WnState, partial) == 256, "WnState layout");
static_assert(sizeof(WnState) % 256 == 0, "WnState size");

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // 16 bytes at any float boundary
__device__ __forceinline__ f4u ld4(const float* p) { return *reinterpret_cast<const f4u*>(p); }
__device__ __forceinline__ void st4(float* p, f4u v) { *reinterpret_cast<f4u*>(p) = v; }

// The elements [0, n) as: head [0, h) up to `align_to`'s next 16-byte boundary, groups of four from h
// (grid-strided, four(i) handles i .. i + 3), and the < 4 leftover ones; one(i) handles a single element.
template <class One, class Four>
__device__ __forceinline__ void strips(size_t n, const void* align_to, One one, Four four) {
  const size_t lead = (4u - (unsigned)(((uintptr_t)align_to >> 2) & 3u)) & 3u;
  const size_t h = lead < n ? lead : n;
  const size_t nv = (n - h) >> 2;
  const size_t tid = blockIdx.x * 256ull + threadIdx.x, nt = 256ull * gridDim.x;
  for (size_t v = tid; v < nv; v += nt) four(h + 4 * v);
  const size_t tail0 = h + 4 * nv;
  if (tid < h) one(tid);
  else if (tid - h < n - tail0) one(tail0 + (tid - h));
}

int strip_blocks(size_t n, int cap) { return (int)std::max<size_t>(1, std::min<size_t>(cap, (n / 4 + 255) / 256)); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- init / mode
__global__ __launch_bounds__(256) void wn_copy(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  strips(n, dst, [&](size_t i) { dst[i] = src[i]; }, [&](size_t i) { st4(dst + i, ld4(src + i)); });
}

__global__ __launch_bounds__(256) void wn_fill(float* __restrict__ dst, float v, size_t n) {
  const f4u v4 = {v, v, v, v};
  strips(n, dst, [&](size_t i) { dst[i] = v; }, [&](size_t i) { st4(dst + i, v4); });
}

// ---------------------------------------------------------------- Sample()
__global__ void wn_tick(WnState* st) { st->t_sample += 1u; }

// parameters = mu + sd * N(0, 1), sd = exp(s)^0.5 (adaptive) or the scalar sigma (fixed: s == nullptr)
__global__ __launch_bounds__(256) void wn_sample(const float* __restrict__ mu, const float* __restrict__ s,
                                                 float* __restrict__ p, size_t n, const WnState* st, float sigma,
                                                 unsigned long long seed) {
  const unsigned long long key = noise_key(seed, st->t_sample);
  auto draw = [&](size_t i, float m, float si) {
    const float sd = s ? sqrtf(expf(si)) : sigma;
    return noise_normal(key, i) * sd + m;
  };
  strips(
      n, p, [&](size_t i) { p[i] = draw(i, mu[i], s ? s[i] : 0.f); },
      [&](size_t i) {
        const f4u m = ld4(mu + i);
        f4u sv = {0.f, 0.f, 0.f, 0.f};
        if (s) sv = ld4(s + i);
        f4u o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = draw(i + k, m[k], sv[k]);
        st4(p + i, o);
      });
}

// ---------------------------------------------------------------- backward: reduction pass
// partial[k][block]: this block's share of the kSums sums (p read only with weight decay, mu and s only when the
// KL term is on); pointers that are not read are nullptr
__global__ __launch_bounds__(256) void wn_reduce(const float* __restrict__ g, const float* __restrict__ p,
                                                 const float* __restrict__ mu, const float* __restrict__ s, size_t n,
                                                 WnState* st) {
  __shared__ double red[kSums][4];
  double q[kSums] = {0., 0., 0., 0., 0., 0.};
  const double c = mu ? (double)mu[0] : 0.;
  auto acc = [&](float gi, float pi, float mi, float si) {
    q[0] += (double)gi * (double)gi;
    q[1] += (double)pi * (double)pi;
    const double d = (double)mi - c;
    q[2] += d;
    q[3] += d * d;
    if (s) {
      q[4] += (double)expf(si);
      q[5] += (double)si;
    }
  };
  strips(
      n, g, [&](size_t i) { acc(g[i], p ? p[i] : 0.f, mu ? mu[i] : 0.f, s ? s[i] : 0.f); },
      [&](size_t i) {
        const f4u z = {0.f, 0.f, 0.f, 0.f};
        const f4u gv = ld4(g + i);
        f4u pv = z, mv = z, sv = z;
        if (p) pv = ld4(p + i);
        if (mu) mv = ld4(mu + i);
        if (s) sv = ld4(s + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc(gv[k], pv[k], mv[k], sv[k]);
      });
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    const double w = wave_sum_d(q[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < kSums)
    st->partial[threadIdx.x][blockIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// ---------------------------------------------------------------- backward: finalise block
// One block: combine the partials (fixed order), then thread 0 applies opt_finalize's rules (gradient norm, clip
// factor, gradient-noise t and sigma, the skip decision on the context's status words / skip_flag) and
// AdaptiveWeightNoise:updateOutput (:63-80).  out[6] = {L, nll_mean (+ L2), KL, ||g||, alpha_mu, alpha_sigma2};
// a skipped call writes out[3] only and leaves the counters alone.
__global__ __launch_bounds__(256) void wn_finalize(WnState* st, int nb, size_t n, const float* mu, int kl,
                                                   float lambda, float maxnorm, float wd, float eta, float gamma,
                                                   const float* nll, int B, float* out, const unsigned* status,
                                                   const float* skip_flag) {
  __shared__ double red[kSums][4];
  __shared__ double tot[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    double a = 0.;
    for (int i = threadIdx.x; i < nb; i += 256) a += st->partial[k][i];
    a = wave_sum_d(a);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x < kSums)
    tot[threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const bool skip = (status && ((__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) |
                                 __hip_atomic_load(status + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) != 0u)) ||
                    (skip_flag && *skip_flag != 0.f);
  st->skip = skip ? 1.f : 0.f;
  const float gn = (float)sqrt(tot[0]);
  out[3] = gn;
  if (skip) return;
  st->clip = gn > maxnorm ? maxnorm / gn : 1.f;
  if (eta != 0.f) {  // gradnoise.t = (gradnoise.t or 0) + 1; sigma = (eta / (1 + t)^gamma)^0.5
    const unsigned t = st->t_gradnoise + 1u;
    st->t_gradnoise = t;
    st->gn_sigma = (float)sqrt((double)eta / pow(1.0 + (double)t, (double)gamma));
  }
  const double dn = (double)n;
  double alpha_mu = 0., alpha_s2 = 1., KL = 0.;  // the module's values before any updateOutput (:8-9)
  if (kl) {
    const double sd = tot[2];
    alpha_mu = (double)mu[0] + sd / dn;
    const double spread = fmax(0., tot[3] - sd * sd / dn);  // sum (mu - alpha_mu)^2
    alpha_s2 = fmax(1e-12, tot[4] / dn + spread / dn);
    KL = 0.5 * (dn * log(alpha_s2) - tot[5]) + 0.5 / alpha_s2 * spread + 0.5 / alpha_s2 * tot[4] - 0.5 * dn;
  }
  st->alpha_mu = alpha_mu;
  st->kl_mu = kl ? (float)((double)lambda / alpha_s2) : 0.f;
  st->kl_s = kl ? (float)((double)lambda * 0.5 / alpha_s2) : 0.f;
  double nllm = 0.;
  for (int b = 0; b < B; ++b) nllm += (double)nll[b];
  nllm /= (double)B;
  if (wd != 0.f) nllm += 0.5 * (double)wd * tot[1];  // nll + 0.5 weightDecay ||parameters||^2 (timit.lua:306)
  out[0] = (float)(kl ? (double)lambda * KL + nllm : nllm);
  out[1] = (float)nllm;
  out[2] = (float)KL;
  out[4] = (float)alpha_mu;
  out[5] = (float)alpha_s2;
}

// ---------------------------------------------------------------- backward: elementwise pass
// g <- clip, + wd * p, + noise in place (as opt_adadelta leaves it); then adaptive (s != nullptr):
// gw[i] = gradmu, gw[n + i] = grads; fixed: gw[i] = g.
__global__ __launch_bounds__(256) void wn_grads(float* __restrict__ g, const float* __restrict__ p,
                                                const float* __restrict__ mu, const float* __restrict__ s,
                                                float* __restrict__ gw, size_t n, const WnState* st, float wd,
                                                int noise, unsigned long long seed, float lambda) {
  if (st->skip != 0.f) return;
  const float clip = st->clip;
  const float sigma = noise ? st->gn_sigma : 0.f;
  const unsigned long long key = noise ? noise_key(seed, st->t_gradnoise) : 0ull;
  const float kl_mu = st->kl_mu, kl_s = st->kl_s, half_lambda = (s && lambda > 0.f) ? 0.5f * lambda : 0.f;
  const double alpha_mu = st->alpha_mu;
  float* __restrict__ gs = gw + n;
  auto grad = [&](size_t i, float gi, float pi) {
    if (clip != 1.f) gi = gi * clip;
    if (wd != 0.f) gi = gi + wd * pi;
    if (noise) gi = gi + noise_normal(key, i) * sigma;
    return gi;
  };
  // (mu - alpha_mu) in double: alpha_mu rounded to fp32 would cost 1e-7 |alpha_mu| / std(mu) of the KL term
  auto gmu = [&](float gi, float mi) { return (float)((double)mi - alpha_mu) * kl_mu + gi; };
  auto gsv = [&](float gi, float si) {
    const float e = expf(si);
    return (e * kl_s - half_lambda) + 0.5f * (gi * gi) * e;
  };
  strips(
      n, g,
      [&](size_t i) {
        const float gi = grad(i, g[i], p ? p[i] : 0.f);
        g[i] = gi;
        if (s) {
          gw[i] = gmu(gi, mu[i]);
          gs[i] = gsv(gi, s[i]);
        } else {
          gw[i] = gi;
        }
      },
      [&](size_t i) {
        f4u gv = ld4(g + i);
        f4u pv = {0.f, 0.f, 0.f, 0.f};
        if (p) pv = ld4(p + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[k] = grad(i + k, gv[k], pv[k]);
        st4(g + i, gv);
        if (s) {
          const f4u mv = ld4(mu + i), sv = ld4(s + i);
          f4u a, b;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            a[k] = gmu(gv[k], mv[k]);
            b[k] = gsv(gv[k], sv[k]);
          }
          st4(gw + i, a);
          st4(gs + i, b);
        } else {
          st4(gw + i, gv);
        }
      });
}

}  // namespace

size_t wnoise_state_bytes() { return sizeof(WnState); }

int wnoise_state_reset(hipStream_t st, void* state) {
  S2S_TRY(zero_async(st, state, sizeof(WnState)));
  return 0;
}

int wnoise_set_steps(hipStream_t st, void* state, unsigned t_sample, unsigned t_gradnoise) {
  WnState* s = static_cast<WnState*>(state);
  S2S_TRY(fill_u32_async(st, &s->t_sample, t_sample, 1));
  S2S_TRY(fill_u32_async(st, &s->t_gradnoise, t_gradnoise, 1));
  return 0;
}

// mu <- parameters; adaptive: s <- log(sigma_init^2) (AdaptiveWeightNoise.lua:40-56); fixed: weight <- parameters
// (WeightNoise.lua:8)
int wnoise_init(hipStream_t st, const WnoiseConfig& c, const float* params, float* weight, size_t n) {
  const int nb = strip_blocks(n, 2048);
  hipLaunchKernelGGL(wn_copy, dim3(nb), dim3(256), 0, st, weight, params, n);
  if (c.adaptive)
    hipLaunchKernelGGL(wn_fill, dim3(nb), dim3(256), 0, st, weight + n,
                       (float)std::log((double)c.sigma * (double)c.sigma), n);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

int wnoise_sample(hipStream_t st, const WnoiseConfig& c, const float* weight, float* params, size_t n, void* state) {
  WnState* s = static_cast<WnState*>(state);
  hipLaunchKernelGGL(wn_tick, dim3(1), dim3(1), 0, st, s);
  hipLaunchKernelGGL(wn_sample, dim3(strip_blocks(n, 2048)), dim3(256), 0, st, weight,
                     c.adaptive ? weight + n : nullptr, params, n, s, c.sigma, c.sample_seed);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

int wnoise_backward(hipStream_t st, const WnoiseConfig& c, const float* weight, const float* params, float* grads,
                    float* gradWeight, size_t n, const float* nll, int B, void* state, float* out,
                    const unsigned* status, const float* skip_flag) {
  WnState* s = static_cast<WnState*>(state);
  const int kl = c.adaptive && c.lambda > 0.f;
  const int noise = c.gradnoise_eta != 0.f;
  const float* p = c.weightDecay != 0.f ? params : nullptr;
  const int nb = strip_blocks(n, kRedBlocks);
  hipLaunchKernelGGL(wn_reduce, dim3(nb), dim3(256), 0, st, grads, p, kl ? weight : nullptr,
                     kl ? weight + n : nullptr, n, s);
  hipLaunchKernelGGL(wn_finalize, dim3(1), dim3(256), 0, st, s, nb, n, weight, kl, c.lambda, c.maxnorm,
                     c.weightDecay, c.gradnoise_eta, c.gradnoise_gamma, nll, B, out, status, skip_flag);
  hipLaunchKernelGGL(wn_grads, dim3(strip_blocks(n, 2048)), dim3(256), 0, st, grads, p, weight,
                     c.adaptive ? weight + n : nullptr, gradWeight, n, s, c.weightDecay, noise, c.gradnoise_seed,
                     c.lambda);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

// parameters <- Mode() = mu (AdaptiveWeightNoise.lua:58-61) / weight (WeightNoise.lua:24-26)
int wnoise_mode(hipStream_t st, const float* weight, float* params, size_t n) {
  hipLaunchKernelGGL(wn_copy, dim3(strip_blocks(n, 2048)), dim3(256), 0, st, params, weight, n);
  S2S_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace s2s
