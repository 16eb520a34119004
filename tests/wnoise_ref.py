"""float64 restatement of the reference's weight-noise modules and the trainer code around them, for the
weight-noise tests (plain numpy; not a test module).

  WeightNoise.lua, AdaptiveWeightNoise.lua            the two modules
  timit/timit.lua:190-205, 241-252, 291-333, 375-379  how the trainer wires them

The normal draws are the device's counter-based ones (oracle.s2s_oracle.gradient_noise restates the generator),
keyed on (sample_seed, t_s) for Sample() and (gradnoise_seed, gradnoise.t) for the gradient noise.
"""
import numpy as np

from oracle.s2s_oracle import gradient_noise

EPS = 1e-12  # AdaptiveWeightNoise.lua:3


def init_weight(params, adaptive, sigma_init=1.0):
    """AdaptiveWeightNoise:initialize (AdaptiveWeightNoise.lua:40-56): mu <- parameters, s <- log(sigma_init^2);
    WeightNoise:__init (WeightNoise.lua:8): weight <- parameters."""
    p = np.asarray(params, dtype=np.float64)
    if not adaptive:
        return p.copy()
    return np.concatenate([p, np.full(p.size, np.log(sigma_init ** 2))])


def sample(weight, n, adaptive, sigma, seed, t):
    """Sample() of call t (AdaptiveWeightNoise.lua:27-38: sigma = exp(s)^0.5, sample = randn * sigma + mu;
    WeightNoise.lua:17-22: sample = randn * sigma + weight)."""
    z = gradient_noise(n, seed, t)
    if adaptive:
        mu, s = weight[:n], weight[n:]
        return z * np.sqrt(np.exp(s)) + mu
    return z * sigma + weight


def alphas(mu, s):
    """AdaptiveWeightNoise.lua:70-71 (and again :90-91): alpha_mu = mean(mu),
    alpha_sigma2 = max(eps, mean(exp s) + sum((mu - alpha_mu)^2) / n)."""
    n = mu.size
    alpha_mu = mu.mean()
    alpha_sigma2 = max(EPS, np.exp(s).mean() + ((mu - alpha_mu) ** 2).sum() / n)
    return alpha_mu, alpha_sigma2


def kl(mu, s):
    """AdaptiveWeightNoise.lua:72-74 with the alphas of :70-71 recomputed from (mu, s)."""
    n = mu.size
    alpha_mu, alpha_sigma2 = alphas(mu, s)
    KL = 0.5 * (n * np.log(alpha_sigma2) - s.sum())
    KL = KL + 0.5 / alpha_sigma2 * ((mu - alpha_mu) ** 2).sum()
    KL = KL + 0.5 / alpha_sigma2 * np.exp(s).sum() - n / 2
    return KL


def kl_grads(mu, s, lam):
    """The KL part of accGradParameters (AdaptiveWeightNoise.lua:92-93): what is added to gradOutput / dLNds."""
    alpha_mu, alpha_sigma2 = alphas(mu, s)
    gradmu = (mu - alpha_mu) / alpha_sigma2 * lam
    grads = np.exp(s) * (lam * 0.5 / alpha_sigma2) - lam * 0.5
    return gradmu, grads


def trainer_gradient(g, p, st, maxnorm=1e20, weightDecay=0.0, gradnoise_eta=0.0, gradnoise_gamma=0.55,
                     gradnoise_seed=0x5EED):
    """timit.lua:297-315 on the (already 1/B-scaled) gradient g, in place: global-norm clip (:297-302), L2 on the
    sampled parameters p (:305-308), gradient noise (:310-315; st["gradnoise_t"] is gradnoise.t).
    Returns (||g|| before clipping, the L2 term added to nll)."""
    gn = float(np.sqrt((g * g).sum()))
    if gn > maxnorm:
        g *= maxnorm / gn
    l2 = 0.0
    if weightDecay > 0:
        l2 = 0.5 * weightDecay * float((p * p).sum())
        g += weightDecay * p
    if gradnoise_eta != 0:
        t = st["gradnoise_t"] = st.get("gradnoise_t", 0) + 1
        g += gradient_noise(g.size, gradnoise_seed, t) * (gradnoise_eta / (1 + t) ** gradnoise_gamma) ** 0.5
    return gn, l2


def backward(weight, p, g, nll, st, adaptive, lam=1.0, **trainer):
    """timit.lua:291-333 after the model's backward: nll (B,) -> mean (:292-295), trainer_gradient on g in place,
    then forward(nll) + backward(nll, gradients) of the module.
    adaptive: updateOutput (AdaptiveWeightNoise.lua:63-80), accGradParameters (:82-104);
    fixed: L = nll (WeightNoise.lua:28-31), gradWeight = g (:33-35 after zeroGradParameters, timit.lua:235-237).
    Returns dict(L, nll, KL, gradnorm, alpha_mu, alpha_sigma2, gradWeight); alpha_* / KL are the module's
    untouched 0 / 1 / 0 when the KL term is off."""
    n = g.size
    gn, l2 = trainer_gradient(g, p, st, **trainer)
    nllm = float(np.mean(nll)) + l2
    out = dict(nll=nllm, KL=0.0, gradnorm=gn, alpha_mu=0.0, alpha_sigma2=1.0)
    if not adaptive:
        out.update(L=nllm, gradWeight=g.copy())
        return out
    mu, s = weight[:n], weight[n:]
    dLNds = 0.5 * g ** 2 * np.exp(s)                       # :87
    if lam > 0:
        out["alpha_mu"], out["alpha_sigma2"] = alphas(mu, s)
        out["KL"] = kl(mu, s)
        out["L"] = lam * out["KL"] + nllm                  # :75
        kmu, ks = kl_grads(mu, s, lam)
        out["gradWeight"] = np.concatenate([kmu + g, ks + dLNds])   # :92-97
    else:
        out["L"] = nllm                                    # :77
        out["gradWeight"] = np.concatenate([g, dLNds])     # :99-100
    return out
