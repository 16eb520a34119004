"""CPU-side checks of the weight-noise work: the float64 restatement the GPU tests compare against
(tests/wnoise_ref.py) is self-consistent, and the s2s_wnoise_* entry points of the built library report bad
arguments instead of aborting.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import wnoise_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fd(f, x, h):
    """Central finite differences of the scalar f at x, one coordinate at a time."""
    g = np.zeros_like(x)
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = h
        g[i] = (f(x + e) - f(x - e)) / (2 * h)
    return g


@pytest.mark.parametrize("mean", [0.0, 3.0])
def test_kl_gradients_are_the_derivatives_of_kl(mean):
    """gradmu - g and grads - dLNds (AdaptiveWeightNoise.lua:92-93) are the derivatives of lambda * KL(mu, s) with
    alpha_mu / alpha_sigma2 recomputed at every point: the alphas minimise the KL, so the total derivative equals
    the partial derivative the reference codes.  n = 50, float64, 1e-6 relative."""
    n, lam = 50, 1.0 / 32
    rng = np.random.default_rng(3)
    mu = mean + rng.standard_normal(n) * 0.08
    s = np.log(rng.uniform(0.01, 0.05, n) ** 2)
    gmu, gs = ref.kl_grads(mu, s, lam)
    fd_mu = _fd(lambda m: lam * ref.kl(m, s), mu, 1e-5)
    fd_s = _fd(lambda v: lam * ref.kl(mu, v), s, 1e-5)
    assert np.abs(gmu - fd_mu).max() <= 1e-6 * np.abs(fd_mu).max()
    assert np.abs(gs - fd_s).max() <= 1e-6 * np.abs(fd_s).max()
    # and through backward(): gradWeight - [g ; dLNds] is that KL part, L = lambda KL + mean nll
    g = rng.standard_normal(n) * 1e-2
    nll = rng.uniform(1, 2, 4)
    out = ref.backward(np.concatenate([mu, s]), mu, g.copy(), nll, {}, True, lam)
    dLNds = 0.5 * g ** 2 * np.exp(s)
    assert np.abs(out["gradWeight"][:n] - g - fd_mu).max() <= 1e-6 * np.abs(fd_mu).max()
    assert np.abs(out["gradWeight"][n:] - dLNds - fd_s).max() <= 1e-6 * np.abs(fd_s).max()
    assert abs(out["L"] - (lam * ref.kl(mu, s) + nll.mean())) <= 1e-12 * abs(out["L"])


def test_kl_clamp_case():
    """All mu equal and s = -40: mean(exp s) + spread = 4e-18 < eps, so alpha_sigma2 is the clamp 1e-12
    (AdaptiveWeightNoise.lua:71).  With alpha_sigma2 pinned the coded gradients are the derivatives of the KL
    with the alphas held fixed (the clamp has no derivative), which is what finite differences at a pinned alpha
    give."""
    n, lam = 50, 1.0 / 32
    mu = np.full(n, 0.25)
    s = np.full(n, -40.0)
    a_mu, a_s2 = ref.alphas(mu, s)
    assert a_mu == 0.25 and a_s2 == ref.EPS
    want = 0.5 * (n * np.log(1e-12) + 40.0 * n) + 0.5e12 * n * np.exp(-40.0) - n / 2
    assert abs(ref.kl(mu, s) - want) <= 1e-12 * abs(want)
    gmu, gs = ref.kl_grads(mu, s, lam)
    assert np.all(gmu == 0.0)

    def kl_pinned(m, v):  # :72-74 at the clamped alpha_sigma2 and the mean of the unperturbed mu
        return (0.5 * (n * np.log(a_s2) - v.sum()) + 0.5 / a_s2 * ((m - a_mu) ** 2).sum()
                + 0.5 / a_s2 * np.exp(v).sum() - n / 2)

    fd_s = _fd(lambda v: lam * kl_pinned(mu, v), s, 1e-4)
    assert np.abs(gs - fd_s).max() <= 1e-6 * np.abs(fd_s).max()


def test_sample_restates_the_modules():
    """Sample() at sigma -> the module's mode; the draws of two calls differ and the adaptive / fixed forms agree
    when exp(s)^0.5 equals the fixed sigma."""
    n = 63
    rng = np.random.default_rng(0)
    p = rng.standard_normal(n)
    w = ref.init_weight(p, True, 0.075)
    assert np.array_equal(w[:n], p) and np.allclose(np.exp(w[n:]) ** 0.5, 0.075, rtol=1e-14)
    a = ref.sample(w, n, True, None, 11, 1)
    b = ref.sample(ref.init_weight(p, False), n, False, 0.075, 11, 1)
    assert np.allclose(a, b, rtol=0, atol=1e-15)
    assert not np.array_equal(a, ref.sample(w, n, True, None, 11, 2))
    assert 0.5 < np.std((a - p) / 0.075) < 1.5


# ------------------------------------------------------------------ host ABI (ctypes on the built library)

def test_wnoise_state_bytes():
    from s2s_amd import _lib
    nbytes = _lib.lib.s2s_wnoise_state_bytes()
    assert nbytes > 0 and nbytes % 256 == 0


def _cfg(_lib, adaptive=1, lam=1 / 32, sigma=0.075, maxnorm=1.0, wd=0.0, eta=0.0, gseed=1, sseed=2):
    return _lib.s2s_wnoise_config(adaptive, lam, sigma, maxnorm, wd, eta, 0.55, gseed, sseed)


def test_wnoise_bad_arguments_are_errors_not_aborts():
    """Null pointers, n = 0, B = 0, a bad config and a null context come back as error codes with a message.
    The non-null pointers below are never dereferenced: every call fails its argument checks (or the null
    context) on the host first."""
    from s2s_amd import _lib
    lib = _lib.lib
    cfg = ctypes.byref(_cfg(_lib))
    fake = ctypes.c_void_p(4096)

    def err():
        return lib.s2s_last_error().decode()

    assert lib.s2s_wnoise_reset(None, None, None) != 0 and "wnoise" in err()
    assert lib.s2s_wnoise_set_steps(None, None, None, 1, 2) != 0 and "wnoise" in err()
    assert lib.s2s_wnoise_init(None, None, None, fake, fake, 8) != 0 and "null config" in err()
    assert lib.s2s_wnoise_init(None, None, cfg, None, fake, 8) != 0 and "wnoise_init" in err()
    assert lib.s2s_wnoise_init(None, None, cfg, fake, fake, 0) != 0 and "wnoise_init" in err()
    assert lib.s2s_wnoise_sample(None, None, cfg, fake, fake, 0, fake) != 0 and "wnoise_sample" in err()
    assert lib.s2s_wnoise_sample(None, None, cfg, fake, None, 8, fake) != 0 and "wnoise_sample" in err()
    assert lib.s2s_wnoise_sample(None, None, cfg, fake, fake, 8, None) != 0 and "wnoise_sample" in err()
    bw = (fake, fake, fake, fake, 8, fake, 4, fake, fake)
    for hole in (0, 1, 2, 3, 5, 7, 8):
        args = list(bw)
        args[hole] = None
        assert lib.s2s_wnoise_backward(None, None, cfg, *args) != 0 and "wnoise_backward" in err(), hole
        assert lib.s2s_wnoise_backward_flag(None, None, cfg, *args, None) != 0 and "wnoise_backward" in err(), hole
    assert lib.s2s_wnoise_backward(None, None, cfg, fake, fake, fake, fake, 0, fake, 4, fake, fake) != 0
    assert "wnoise_backward" in err()
    assert lib.s2s_wnoise_backward(None, None, cfg, fake, fake, fake, fake, 8, fake, 0, fake, fake) != 0
    assert "B must be positive" in err()
    assert lib.s2s_wnoise_mode(None, None, cfg, None, fake, 8) != 0 and "wnoise_mode" in err()
    assert lib.s2s_wnoise_mode(None, None, cfg, fake, fake, 0) != 0 and "wnoise_mode" in err()
    # a bad config: adaptive with sigma_init = 0 (log 0), a non-positive maxnorm, equal seeds with both noises on
    for bad in (_cfg(_lib, sigma=0.0), _cfg(_lib, maxnorm=0.0), _cfg(_lib, eta=1e-3, gseed=7, sseed=7),
                _cfg(_lib, adaptive=2)):
        assert lib.s2s_wnoise_sample(None, None, ctypes.byref(bad), fake, fake, 8, fake) != 0
        assert "wnoise" in err()
    # everything else valid: the null context is what is reported
    assert lib.s2s_wnoise_sample(None, None, cfg, fake, fake, 8, fake) != 0 and "null context" in err()
    assert lib.s2s_wnoise_backward(None, None, cfg, *bw) != 0 and "null context" in err()
    assert lib.s2s_wnoise_reset(None, None, fake) != 0 and "null context" in err()


def test_wnoise_config_matches_header_typedef():
    """The ctypes mirror of s2s_wnoise_config lists the header's fields in order, with the header's types."""
    from s2s_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "s2s_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*s2s_wnoise_config;", hdr).group(1)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "unsigned long long": ctypes.c_ulonglong}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"((?:unsigned long long|int|float))\s+(.*)$", decl).groups()
        fields += [(nm.strip(), ctype[typ]) for nm in names.split(",")]
    assert list(_lib.s2s_wnoise_config._fields_) == fields


def test_python_wrapper_refuses_equal_seeds_before_touching_the_device():
    """Both noises on with one seed would draw the same normals twice: ValueError from the constructor."""
    torch = pytest.importorskip("torch")
    from s2s_amd import optim

    class Flat:  # stands in for a flat CUDA tensor: the seed check comes right after the tensor checks
        is_cuda, dtype, shape = True, torch.float32, (8,)

        def is_contiguous(self):
            return True

        def dim(self):
            return 1

        def numel(self):
            return 8

    with pytest.raises(ValueError, match="sample_seed"):
        optim.AdaptiveWeightNoise(params=Flat(), grads=Flat(), gradnoise_eta=1e-3, gradnoise_seed=5, sample_seed=5)
    with pytest.raises(ValueError, match="sample_seed"):
        optim.WeightNoise(params=Flat(), grads=Flat(), gradnoise_eta=1e-3, gradnoise_seed=5, sample_seed=5)
