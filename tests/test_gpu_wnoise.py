"""Weight noise / adaptive weight noise on the device (s2s_wnoise_*, s2s_amd.optim.WeightNoise /
AdaptiveWeightNoise) against tests/wnoise_ref.py, the float64 restatement of WeightNoise.lua,
AdaptiveWeightNoise.lua and timit/timit.lua:291-333.

Tolerances (fp32 on the GPU vs float64), max-norm relative as in test_gpu_parity.py:
  samples, gradWeight, the in-place g                  1e-5   (the bar test_optimizer_step_matches_oracle holds
                                                                this normal generator to); also each half of
                                                                gradWeight on its own scale (see run_backward)
  gradnorm, alpha_sigma2, nll_mean, L                   1e-5 relative
  alpha_mu                                              1e-6 * max|mu| absolute
  KL                                                    1e-6 * n absolute (about ten times the worst case of fp32
                                                        exp rounding carried through 0.5 n log(alpha_sigma2))
"""
import functools

import numpy as np
import pytest
import torch

from oracle import s2s_oracle as orc
import wnoise_ref as ref

pytestmark = pytest.mark.gpu

N_CH = 4_356_222          # the Chorowski flat layout (tests/test_abi.py::test_chorowski_param_count)
SIZES = [1, 63, 257, 4099, N_CH]
OFFSETS = [0, 1, 3]       # floats into a larger buffer: the unaligned head of the 16-byte body
SEED_S, SEED_G = 1234567, 99


@pytest.fixture(scope="module")
def s2s():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import s2s_amd
    return s2s_amd


def cu(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def host(t):
    return t.detach().cpu().double().numpy()


def rel(g, r):
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    assert g.shape == r.shape and np.isfinite(g).all()
    return float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-300))


def sliced(n, off):
    """A length-n view `off` floats into a larger zero buffer."""
    return torch.zeros(n + 8, dtype=torch.float32, device="cuda")[off:off + n]


@functools.lru_cache(maxsize=None)
def inputs(n, kind):
    """fp32 inputs (read-only; shared by the tests).  A: mu ~ N(0, 0.08); B: the offset-mean case mu ~ N(3, 0.01);
    both sigma ~ U(0.01, 0.05), s = log sigma^2; clamp: mu all equal, s = -40.  g ~ 1e-3 N(0, 1) (the optimizer
    test's), p = a sample-like perturbation of mu, nll (B = 4)."""
    rng = np.random.default_rng(1000 + n % 997 + {"A": 0, "B": 1, "clamp": 2}[kind])
    if kind == "clamp":
        mu, s = np.full(n, 0.25), np.full(n, -40.0)
    else:
        mean, std = (0.0, 0.08) if kind == "A" else (3.0, 0.01)
        mu = mean + rng.standard_normal(n) * std
        s = np.log(rng.uniform(0.01, 0.05, n) ** 2)
    g = rng.standard_normal(n) * 1e-3
    p = mu + rng.standard_normal(n) * 0.03
    nll = rng.uniform(1.0, 3.0, 4)
    out = tuple(a.astype(np.float32) for a in (mu, s, g, p, nll))
    for a in out:
        a.setflags(write=False)
    return out


def make(s2s, n, adaptive, off=0, **kw):
    """A module on raw flat buffers that start `off` floats into larger ones."""
    params, grads = sliced(n, off), sliced(n, off)
    cls = s2s.optim.AdaptiveWeightNoise if adaptive else s2s.optim.WeightNoise
    return cls(params=params, grads=grads, sample_seed=SEED_S, gradnoise_seed=SEED_G, **kw)


# --------------------------------------------------------------------------- 1. sample / init / mode

@pytest.mark.parametrize("adaptive", [True, False], ids=["adaptive", "fixed"])
@pytest.mark.parametrize("n", SIZES)
def test_sample_matches_restatement(s2s, n, adaptive):
    """Three consecutive sample() calls (t_s = 1, 2, 3) at every buffer offset equal the restatement's draws keyed
    on (sample_seed, t_s); init sets mu <- parameters, s <- log(sigma_init^2); mode() restores mu bitwise."""
    mu, s, _, _, _ = inputs(n, "A")
    sigma = 0.075
    w64 = np.concatenate([mu, s]).astype(np.float64) if adaptive else mu.astype(np.float64)
    want = [ref.sample(w64, n, adaptive, sigma, SEED_S, t) for t in (1, 2, 3)]
    for off in OFFSETS:
        kw = dict(sigma_init=sigma) if adaptive else dict(sigma=sigma)
        m = make(s2s, n, adaptive, off, **kw)
        m.params.copy_(cu(mu))
        fresh = type(m)(params=m.params, grads=m.grads, sample_seed=SEED_S, **kw)   # init from these parameters
        assert torch.equal(fresh.weight[:n], m.params)
        if adaptive:
            s0 = host(fresh.weight[n:])
            assert np.abs(s0 - np.log(sigma ** 2)).max() <= 1e-6 * abs(np.log(sigma ** 2))
            m.weight.copy_(cu(np.concatenate([mu, s])))
        else:
            assert fresh.weight.numel() == n
            m.weight.copy_(cu(mu))
        for t in range(3):
            m.sample()
            e = rel(host(m.params), want[t])
            print(f"sample n={n} adaptive={adaptive} off={off} t={t + 1}: rel err {e:.3e}")
            assert e <= 1e-5, (off, t, e)
        assert m.steps() == (3, 0)
        m.mode()
        assert torch.equal(m.params, m.weight[:n])


# --------------------------------------------------------------------------- 2. backward

TRAINER = {"off": (1e20, 0.0, 0.0), "clip": (0.5e-2, 0.0, 0.0), "wd": (1e20, 1e-3, 0.0), "all": (0.5e-2, 1e-3, 1e-3)}


def run_backward(s2s, n, kind, adaptive, lam, maxnorm, wd, eta, off=0):
    """backward() on inputs(n, kind) vs the restatement; returns nothing, asserts every bar."""
    mu, s, g, p, nll = inputs(n, kind)
    kw = dict(maxnorm=maxnorm, weightDecay=wd, gradnoise_eta=eta)
    if adaptive:
        m = make(s2s, n, True, off, adalambda=lam, sigma_init=0.075, **kw)
        m.weight.copy_(cu(np.concatenate([mu, s])))
    else:
        m = make(s2s, n, False, off, sigma=0.075, **kw)
        m.weight.copy_(cu(mu))
    m.params.copy_(cu(p))
    m.grads.copy_(cu(g))
    m.backward(cu(nll))
    torch.cuda.synchronize()
    g64 = g.astype(np.float64)
    w64 = np.concatenate([mu, s]).astype(np.float64) if adaptive else mu.astype(np.float64)
    st = {}
    want = ref.backward(w64, p.astype(np.float64), g64, nll.astype(np.float64), st, adaptive, lam, **kw,
                        gradnoise_seed=SEED_G)
    out = host(m.out)
    got = dict(L=out[0], nll=out[1], KL=out[2], gradnorm=out[3], alpha_mu=out[4], alpha_sigma2=out[5])
    tag = f"n={n} {kind} adaptive={adaptive} lam={lam:g} maxnorm={maxnorm:g} wd={wd:g} eta={eta:g} off={off}"
    gw, gwr = host(m.gradWeight), want["gradWeight"]
    errs = {"g": rel(host(m.grads), g64), "gradWeight": rel(gw, gwr), "gradmu": rel(gw[:n], gwr[:n])}
    if adaptive:
        # the s half against its own (much smaller) scale, beyond the whole-vector bar: its KL part is the
        # difference lambda/2 exp(s)/alpha_sigma2 - lambda/2 of two fp32-rounded terms, so four roundings
        # (2^-24 each: the exp, the scalar, the product, the difference) of the larger one are its floor
        # (at n = 1 the two terms are equal and the floor is all there is)
        floor = 4 * 2.0 ** -24 * (lam / 2 if lam > 0 else 0.0) * max(1.0, float(np.exp(s.astype(np.float64)).max())
                                                                     / want["alpha_sigma2"])
        e_s = float(np.abs(gw[n:] - gwr[n:]).max())
        print(f"  grads half: max err {e_s:.3e}, bar {1e-5 * np.abs(gwr[n:]).max() + floor:.3e}")
        assert e_s <= 1e-5 * np.abs(gwr[n:]).max() + floor, (tag, e_s)
    for k in ("gradnorm", "alpha_sigma2", "nll", "L"):
        errs[k] = abs(got[k] - want[k]) / abs(want[k])
    kl_err = abs(got["KL"] - want["KL"])
    amu_err = abs(got["alpha_mu"] - want["alpha_mu"])
    print(f"backward {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f" |dKL|/n {kl_err / n:.2e} (KL/n {want['KL'] / n:.3f}) |dalpha_mu| {amu_err:.2e}")
    for k, v in errs.items():
        assert v <= 1e-5, (tag, k, v)
    assert amu_err <= 1e-6 * np.abs(mu).max(), (tag, amu_err)
    assert kl_err <= 1e-6 * n, (tag, kl_err)
    if adaptive and lam > 0 and n > 1:
        # the inputs make the absolute KL bar at most 1e-5 relative.  n = 1 is exempt by construction: there
        # mu = alpha_mu and exp(s) = alpha_sigma2, so KL = 0 identically and only the absolute bar can hold.
        assert want["KL"] >= 0.1 * n, (tag, want["KL"])
    assert m.steps() == (0, 1 if eta else 0)


@pytest.mark.parametrize("lam", [0.0, 1.0 / 32], ids=["lam0", "lam1/32"])
@pytest.mark.parametrize("trainer", list(TRAINER))
@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("n", SIZES)
def test_backward_matches_restatement(s2s, n, kind, trainer, lam):
    """Adaptive backward on input A (mu ~ N(0, 0.08), KL/n = 1.14) and the offset-mean input B (mu ~ N(3, 0.01),
    KL/n = 0.20, where an fp32 one-pass variance is off by 1 %): the optimizer test's (clip, wd, eta) cases x
    lambda in {0, 1/32} at every size.  maxnorm 0.5e-2 clips these gradients (||g|| = 1e-3 sqrt(n)) from n = 63 up;
    the gradient buffer starts n % 4 floats into its allocation, so every head length occurs."""
    run_backward(s2s, n, kind, True, lam, *TRAINER[trainer], off=n % 4)


@pytest.mark.parametrize("n", SIZES)
def test_backward_fixed_mode(s2s, n):
    """WeightNoise: gradWeight = the clipped / decayed / noised g, L = mean nll + the L2 term."""
    run_backward(s2s, n, "A", False, 0.0, *TRAINER["all"], off=(n + 1) % 4)


def test_backward_clamp_case(s2s):
    """mu all equal, s = -40: alpha_sigma2 is the 1e-12 clamp (AdaptiveWeightNoise.lua:71); the shifted sums leave
    the spread exactly 0, so 0.5 / 1e-12 * spread adds nothing to the KL."""
    run_backward(s2s, 257, "clamp", True, 1.0 / 32, *TRAINER["off"], off=1)


# --------------------------------------------------------------------------- 3. skip_flag

@pytest.mark.parametrize("adaptive", [True, False], ids=["adaptive", "fixed"])
def test_skip_flag_leaves_everything_untouched(s2s, adaptive):
    """skip_flag = 1: g, gradWeight and both counters are bitwise untouched (gradnorm is still written); the next
    unskipped call equals the first call of a module that never saw the skipped one."""
    n = 4099
    mu, s, g, p, nll = inputs(n, "A")
    kw = dict(maxnorm=0.5e-2, weightDecay=1e-3, gradnoise_eta=1e-3)
    kw.update(dict(adalambda=1 / 32, sigma_init=0.075) if adaptive else dict(sigma=0.075))

    def fresh():
        m = make(s2s, n, adaptive, 1, **kw)
        m.weight.copy_(cu(np.concatenate([mu, s]) if adaptive else mu))
        m.params.copy_(cu(p))
        m.grads.copy_(cu(g))
        m.gradWeight.fill_(7.0)
        m.set_steps(5, 9)
        return m

    a, b = fresh(), fresh()
    nlld = cu(nll)
    g0, gw0 = a.grads.clone(), a.gradWeight.clone()
    a.backward(nlld, skip_flag=torch.ones(1, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(a.grads, g0) and torch.equal(a.gradWeight, gw0)
    assert a.steps() == (5, 9)
    gn = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    assert abs(a.gradnorm.item() - gn) <= 1e-5 * gn
    assert torch.equal(a.out[:3], torch.zeros(3, device="cuda"))
    zero = torch.zeros(1, device="cuda")
    a.backward(nlld, skip_flag=zero)
    b.backward(nlld)
    torch.cuda.synchronize()
    assert torch.equal(a.grads, b.grads) and torch.equal(a.gradWeight, b.gradWeight) and torch.equal(a.out, b.out)
    assert a.steps() == b.steps() == (5, 10)
    assert not torch.equal(a.grads, g0)


# --------------------------------------------------------------------------- 4. resume

def _iterate(m, g, nll, p_log=None):
    m.sample()
    m.grads.copy_(g)
    m.backward(nll)
    if p_log is not None:
        p_log.append((m.params.clone(), m.grads.clone(), m.gradWeight.clone(), m.out.clone()))


@pytest.mark.parametrize("adaptive", [True, False], ids=["adaptive", "fixed"])
def test_resume_from_state_dict_and_set_steps(s2s, adaptive):
    """state_dict() after two steps, loaded into a fresh module (built with other seeds): its third sample() /
    backward() are bitwise the original's.  The same from set_steps() on a module given the weight by hand."""
    n = 4099
    mu, s, g, p, nll = inputs(n, "A")
    kw = dict(maxnorm=0.5e-2, weightDecay=1e-3, gradnoise_eta=1e-3)
    kw.update(dict(adalambda=1 / 32, sigma_init=0.075) if adaptive else dict(sigma=0.075))
    gd, nlld = cu(g), cu(nll)
    a = make(s2s, n, adaptive, 3, **kw)
    a.weight.copy_(cu(np.concatenate([mu, s]) if adaptive else mu))
    for _ in range(2):
        _iterate(a, gd, nlld)
        a.weight.sub_(0.1 * a.gradWeight)        # any update of the trainable vector
    sd = a.state_dict()
    assert (sd["t_sample"], sd["t_gradnoise"]) == (2, 2)
    assert (sd["sample_seed"], sd["gradnoise_seed"]) == (SEED_S, SEED_G)
    cls = type(a)
    b = cls(params=sliced(n, 3), grads=sliced(n, 3), sample_seed=1, gradnoise_seed=2, **kw)
    b.load_state_dict(sd)
    c = make(s2s, n, adaptive, 3, **kw)
    c.weight.copy_(a.weight)
    c.set_steps(2, 2)
    logs = [[], [], []]
    for m, log in zip((a, b, c), logs):
        _iterate(m, gd, nlld, log)
    torch.cuda.synchronize()
    for other in logs[1:]:
        for x, y in zip(logs[0][0], other[0]):
            assert torch.equal(x, y)
    assert a.steps() == b.steps() == c.steps() == (3, 3)


# --------------------------------------------------------------------------- 5. repeatability and capture

def test_two_runs_are_bitwise_equal(s2s):
    """Same state, same inputs: sample() and backward() repeat bitwise (fixed-order double reduction), at the
    Chorowski size where the reduction spans every block."""
    mu, s, g, p, nll = inputs(N_CH, "B")
    gd, nlld = cu(g), cu(nll)
    logs = []
    for _ in range(2):
        m = make(s2s, N_CH, True, 1, adalambda=1 / 32, sigma_init=0.075, maxnorm=0.5e-2, weightDecay=1e-3,
                 gradnoise_eta=1e-3)
        m.weight.copy_(cu(np.concatenate([mu, s])))
        log = []
        for _ in range(2):
            _iterate(m, gd, nlld, log)
        logs.append(log)
    torch.cuda.synchronize()
    for x, y in zip(logs[0], logs[1]):
        for u, v in zip(x, y):
            assert torch.equal(u, v)


@pytest.mark.parametrize("adaptive", [True, False], ids=["adaptive", "fixed"])
def test_graph_capture_replays_the_counters(s2s, adaptive):
    """sample + backward + Adadelta.step on fixed g / nll buffers captured in one torch.cuda.graph (a linear chain):
    three replays equal three eager iterations bitwise, the device counters advancing inside the graph."""
    n = 4099
    mu, s, g, p, nll = inputs(n, "A")
    kw = dict(maxnorm=0.5e-2, weightDecay=1e-3, gradnoise_eta=1e-3)
    kw.update(dict(adalambda=1 / 32, sigma_init=0.075) if adaptive else dict(sigma=0.075))
    gd, nlld = cu(g), cu(nll)

    def build():
        m = make(s2s, n, adaptive, 1, **kw)
        m.weight.copy_(cu(np.concatenate([mu, s]) if adaptive else mu))
        return m, s2s.optim.Adadelta(params=m.weight, grads=m.gradWeight, ctx=m.ctx)

    def fn(m, opt):
        m.sample()
        torch.mul(gd, 1.0, out=m.grads)      # a kernel node (exact), not a memcpy node
        m.backward(nlld)
        opt.step()

    fn(*build())                    # a throwaway module: every kernel has run once before the capture
    eager, graphed = build(), build()
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        fn(*graphed)
    torch.cuda.current_stream().wait_stream(side)
    assert graphed[0].steps() == (0, 0)      # capturing ran nothing
    w0 = graphed[0].weight.clone()
    for it in range(3):
        fn(*eager)
        graph.replay()
        torch.cuda.synchronize()
        for name in ("params", "grads", "gradWeight", "weight", "out"):
            assert torch.equal(getattr(eager[0], name), getattr(graphed[0], name)), (it, name)
        assert torch.equal(eager[1].state, graphed[1].state), it
        assert eager[0].steps() == graphed[0].steps() == (it + 1, it + 1)
    assert not torch.equal(graphed[0].weight, w0)


# --------------------------------------------------------------------------- 6. end to end

SMOKE = dict(inputFrameSize=40, hiddenFrameSize=32, outputFrameSize=32, scoreDepth=64, stateDepth=32,
             outputDepth=62, mlpDepth=8, maxoutWindow=7, numLayers=3)


def test_end_to_end_with_the_model_step(s2s):
    """sample -> model.step -> backward on the smoke-sized ChorowskiBaseline (B = 4, L = 32, T = 8) against
    orc.training_step evaluated at the same sampled parameters (float64) followed by the restatement.
    gradmu: the project's 1e-4; grads: 2.5e-4 (the squared gradient doubles 1e-4, a quarter more for the sigma^2
    product); L: 1e-4 relative.  Then three full iterations with the optimizer on weight (column-norm constraint on
    the rows of mu): status 0, finite L, weight changed."""
    B, L, T = 4, 32, 8
    model = s2s.ChorowskiBaseline(s2s.ModelConfig(**SMOKE))
    cfg = orc.ModelConfig(**SMOKE)
    x, labels = orc.synthetic_batch(cfg, B, L, T, seed=1234, pad=4, eos=23)
    xd = torch.tensor(x, dtype=torch.float32, device="cuda")
    ld = torch.tensor(labels, dtype=torch.int32, device="cuda")
    lam = 1.0 / B
    awn = s2s.optim.AdaptiveWeightNoise(model, adalambda=lam, sigma_init=0.01, maxnorm=1.0, weightDecay=1e-4,
                                        sample_seed=SEED_S)
    n = awn.n
    assert awn.params.data_ptr() == model.params.data_ptr() and awn.weight.numel() == 2 * n
    w64 = host(awn.weight)
    awn.sample()
    nll, _ = model.step(xd, ld)
    awn.backward(nll)
    torch.cuda.synchronize()
    p64 = host(model.params)
    assert rel(p64, ref.sample(w64, n, True, None, SEED_S, 1)) <= 1e-5
    nll_ref, G, _, _ = orc.training_step(x, labels, orc.unflatten(p64, cfg), cfg)
    gref = orc.flatten(G, cfg)
    want = ref.backward(w64, p64, gref, np.array([nll_ref]), {}, True, lam, maxnorm=1.0, weightDecay=1e-4)
    gw = host(awn.gradWeight)
    e_mu, e_s = rel(gw[:n], want["gradWeight"][:n]), rel(gw[n:], want["gradWeight"][n:])
    e_L = abs(awn.L.item() - want["L"]) / abs(want["L"])
    print(f"end to end: gradmu {e_mu:.2e} grads {e_s:.2e} L {e_L:.2e} (L {want['L']:.5f}, KL {want['KL']:.3f}, "
          f"gradnorm {want['gradnorm']:.4f})")
    assert e_mu <= 1e-4 and e_s <= 2.5e-4 and e_L <= 1e-4, (e_mu, e_s, e_L)
    mats = s2s.optim.weight_matrices(model.cfg)
    opt = s2s.optim.Adadelta(params=awn.weight, grads=awn.gradWeight, mats=mats, colnormconstr=True, ctx=model.ctx)
    w0 = awn.weight.clone()
    for _ in range(3):
        awn.sample()
        nll, _ = model.step(xd, ld)
        awn.backward(nll)
        opt.step()
    torch.cuda.synchronize()
    assert model.ctx.status(clear=False) == 0
    assert np.isfinite(awn.L.item()) and np.isfinite(host(awn.weight)).all()
    assert not torch.equal(awn.weight, w0)
    mu_now = host(awn.weight[:n])
    for off, r, c in mats:
        assert np.linalg.norm(mu_now[off:off + r * c].reshape(r, c), axis=1).max() <= 1.0 + 1e-5
    awn.mode()
    assert torch.equal(model.params, awn.weight[:n])
