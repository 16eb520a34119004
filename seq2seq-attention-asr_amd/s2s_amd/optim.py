"""Device optimizer step: timit/timit.lua:292-347 on the flat buffers --
global-norm clip, L2, optim.adadelta and TrainUtils.columnNormConstraint -- in one stream-ordered
sequence of kernels (libs2s_hip.so: s2s_optim_adadelta_step), no host round trip.

    opt = Adadelta(model, rho=0.95, eps=1e-8, colnormconstr=True)   # exp_logmel7_..._colnorm.lua
    model.step(x, labels)                                           # grads = mean over the batch
    opt.step()                                                      # x updated in place

Data parallel (one process per GPU): every rank's gradients went into the all-reduce, so a rank whose persistent
launch failed poisons every replica's sum -- all ranks must skip that update together:

    flag = opt.failure_flag()                   # 1.0 on a rank whose step failed (device, stream-ordered)
    dist.reduce_failure_flag(flag)              # MAX over the ranks
    opt.step(skip_flag=flag)                    # skipped on every rank if any rank failed

Weight noise (WeightNoise.lua) and adaptive weight noise (AdaptiveWeightNoise.lua) as the reference trainer wires
them (timit/timit.lua:190-205, 241-252, 291-333, 375-379), on the device (libs2s_hip.so: s2s_wnoise_*):

    awn = AdaptiveWeightNoise(model, adalambda=1/B, sigma_init=0.075, maxnorm=1, ...)
    opt = Adadelta(params=awn.weight, grads=awn.gradWeight, ctx=model.ctx)   # clip / L2 / noise belong to awn
    awn.sample(); nll, _ = model.step(x, y); awn.backward(nll); opt.step()
    awn.mode()   # before evaluation / beam search
"""
import ctypes

import torch

from . import _lib
from ._lib import check, lib
from .nn import dptr, get_context, stream_ptr


def weight_matrices(cfg):
    """(offset, rows, cols) of every module weight of the flat layout (s2s_model_weight_matrices)."""
    from .model import ModelConfig  # noqa: F401
    c = cfg
    d = _lib.s2s_model_dims(1, 1, 1, c.inputFrameSize, c.hiddenFrameSize, c.outputFrameSize, c.numLayers,
                            c.scoreDepth, c.stateDepth, c.outputDepth, c.mlpDepth, c.maxoutWindow, c.penalty, 0.0)
    n = lib.s2s_model_weight_matrices(ctypes.byref(d), None)
    if n < 0:
        check(1)
    buf = (ctypes.c_long * (3 * n))()
    lib.s2s_model_weight_matrices(ctypes.byref(d), buf)
    return [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]


class Adadelta:
    """optim.adadelta with the reference trainer's surroundings (timit/timit.lua:292-347):
    opt.maxnorm (gradient clip), opt.weightDecay (L2), opt.colnormconstr (max row norm 1) and the
    gradient noise table gradnoise = {eta, gamma} (timit.lua:185-189, 310-315; the configs set eta = 0,
    timit.lua's own default is 1e-3).  The noise counter t lives in self.state (checkpointed with it);
    gradnoise_seed must be equal on every data-parallel rank so the replicas stay identical.
    params / grads: flat float32 CUDA tensors (ChorowskiBaseline.getParameters()), or pass the model.
    The update runs on the model's context (or ctx): if that context's failure status is set when the update
    runs on the device (a persistent launch of the step before it timed out), the update is skipped there."""

    def __init__(self, model=None, params=None, grads=None, mats=None, rho=0.95, eps=1e-8, maxnorm=1e20,
                 weightDecay=0.0, colnormconstr=False, colnorm_max=1.0, gradnoise_eta=0.0, gradnoise_gamma=0.55,
                 gradnoise_seed=0x5EED, ctx=None):
        if model is not None:
            params, grads = model.getParameters()
            if mats is None:
                mats = weight_matrices(model.cfg)
        if not (params.is_cuda and params.dtype == torch.float32 and params.is_contiguous()
                and grads.shape == params.shape):
            raise ValueError("params / grads must be flat contiguous float32 CUDA tensors of one size")
        self.params, self.grads = params, grads
        self.n = params.numel()
        self.cfg = _lib.s2s_optim_config(rho, eps, maxnorm, weightDecay, colnorm_max if colnormconstr else 0.0,
                                         gradnoise_eta, gradnoise_gamma, gradnoise_seed)
        mats = list(mats or [])
        self._mats = (ctypes.c_long * max(1, 3 * len(mats)))(*[v for m in mats for v in m])
        self._nmats = len(mats)
        self.state = torch.zeros(lib.s2s_optim_state_bytes(self.n), dtype=torch.uint8, device=params.device)
        self.gradnorm = torch.zeros(1, dtype=torch.float32, device=params.device)
        if ctx is None:
            ctx = getattr(model, "ctx", None) or get_context(params.device.index)
        self.ctx = ctx

    def set_noise_step(self, t, stream=None):
        """gradnoise.t of a resumed run (timit/timit.lua:92, 312): the next step draws with t + 1."""
        st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else stream_ptr()
        check(lib.s2s_optim_set_noise_step(self.ctx.handle, st, dptr(self.state), self.n, int(t)))

    def failure_flag(self, stream=None, out=None):
        """A one-float device tensor: 1.0 if this context's failure status is set when it runs on the stream, else
        0.0 (stream-ordered, no host sync).  Data parallel: all-reduce it across the ranks (dist.reduce_failure_flag)
        and pass it to step(skip_flag=...), so a failure on any rank skips the update on every rank."""
        st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else stream_ptr()
        if out is None:
            out = torch.zeros(1, dtype=torch.float32, device=self.params.device)
        check(lib.s2s_ctx_status_flag(self.ctx.handle, st, dptr(out)))
        return out

    def step(self, stream=None, skip_flag=None):
        """One update; self.gradnorm holds ||g|| before clipping (timit.lua:297 gradnorms).  skip_flag: a one-float
        device tensor (the all-reduced failure_flag of every rank); nonzero when the update runs = skip it."""
        st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else stream_ptr()
        if skip_flag is None:
            check(lib.s2s_optim_adadelta_step(self.ctx.handle, st, ctypes.byref(self.cfg), dptr(self.params),
                                              dptr(self.grads), self.n, dptr(self.state), self._mats, self._nmats,
                                              dptr(self.gradnorm)))
            return
        if not (skip_flag.is_cuda and skip_flag.dtype == torch.float32 and skip_flag.numel() >= 1):
            raise ValueError("skip_flag must be a float32 CUDA tensor")
        check(lib.s2s_optim_adadelta_step_flag(self.ctx.handle, st, ctypes.byref(self.cfg), dptr(self.params),
                                               dptr(self.grads), self.n, dptr(self.state), self._mats, self._nmats,
                                               dptr(self.gradnorm), dptr(skip_flag)))


class _WeightNoiseBase:
    """Shared host side of WeightNoise / AdaptiveWeightNoise: the trainable `weight` and its `gradWeight`, the
    device state block (both counters, the clip / KL scalars) and the six-float device output of backward().
    The trainer's clip (opt.maxnorm), L2 (opt.weightDecay, on the SAMPLED parameters) and gradient noise
    (gradnoise = {eta, gamma}) are applied by backward() to the model gradient before the module sees it
    (timit/timit.lua:297-315), so the optimizer on `weight` must leave them off.

    Three deliberate differences from the reference:
      1. One draw per sample() call.  The reference draws a new sample per utterance inside its per-utterance
         loop (timit.lua:241-252); the step here is batched, so call sample() once per minibatch (the same
         thing at B = 1).
      2. Counter-based draws: element i of call t is noise_normal(key(sample_seed, t), i), the generator of the
         gradient noise with a seed of its own, so every launch geometry and data-parallel rank draws the same
         sample.  With both noises on, sample_seed must differ from gradnoise_seed (ValueError otherwise).
      3. Column-norm constraint: Adadelta(params=weight, ..., mats=weight_matrices(cfg), colnormconstr=True)
         constrains the rows of mu (the matrix offsets index the first n elements); the reference's constraint
         lands on the sampled copy, which the next draw overwrites (timit.lua:344-346)."""

    def __init__(self, adaptive, lam, sigma, model, params, grads, maxnorm, weightDecay, gradnoise_eta,
                 gradnoise_gamma, gradnoise_seed, sample_seed, ctx):
        if model is not None:
            params, grads = model.getParameters()
        if not (params.is_cuda and params.dtype == torch.float32 and params.is_contiguous() and params.dim() == 1
                and grads.shape == params.shape and grads.dtype == torch.float32 and grads.is_contiguous()
                and params.numel() > 0):
            raise ValueError("params / grads must be flat contiguous float32 CUDA tensors of one size")
        if gradnoise_eta != 0 and int(gradnoise_seed) == int(sample_seed):
            raise ValueError("sample_seed must differ from gradnoise_seed when gradient noise is on: equal seeds "
                             "and counters would draw the same normals for both")
        self.params, self.grads = params, grads
        self.n = params.numel()
        self.adaptive = bool(adaptive)
        self.cfg = _lib.s2s_wnoise_config(int(self.adaptive), lam, sigma, maxnorm, weightDecay, gradnoise_eta,
                                          gradnoise_gamma, gradnoise_seed, sample_seed)
        dev = params.device
        m = 2 * self.n if self.adaptive else self.n
        self.weight = torch.empty(m, dtype=torch.float32, device=dev)
        self.gradWeight = torch.zeros(m, dtype=torch.float32, device=dev)
        self.state = torch.zeros(lib.s2s_wnoise_state_bytes(), dtype=torch.uint8, device=dev)
        self.out = torch.zeros(6, dtype=torch.float32, device=dev)
        if ctx is None:
            ctx = getattr(model, "ctx", None) or get_context(dev.index)
        self.ctx = ctx
        check(lib.s2s_wnoise_init(self.ctx.handle, stream_ptr(), ctypes.byref(self.cfg), dptr(params),
                                  dptr(self.weight), self.n))

    # device views of the last backward(): no host sync until the caller reads them
    @property
    def L(self):
        """The loss the optimizer minimises: lambda * KL + nll (adaptive, lambda > 0), else nll (with the L2 term)."""
        return self.out[0:1]

    @property
    def nll(self):
        """Mean nll over the minibatch, plus 0.5 * weightDecay * ||parameters||^2 (timit.lua:292-308)."""
        return self.out[1:2]

    @property
    def KL(self):
        return self.out[2:3]

    @property
    def gradnorm(self):
        """||g|| before clipping (timit.lua:297 gradnorms)."""
        return self.out[3:4]

    @property
    def alpha_mu(self):
        return self.out[4:5]

    @property
    def alpha_sigma2(self):
        return self.out[5:6]

    @staticmethod
    def _st(stream):
        return ctypes.c_void_p(stream.cuda_stream) if stream is not None else stream_ptr()

    def sample(self, stream=None):
        """parameters <- Sample() (AdaptiveWeightNoise.lua:27-38 / WeightNoise.lua:17-22): ONE draw, keyed on
        (sample_seed, the device sample counter after its increment)."""
        check(lib.s2s_wnoise_sample(self.ctx.handle, self._st(stream), ctypes.byref(self.cfg), dptr(self.weight),
                                    dptr(self.params), self.n, dptr(self.state)))

    def backward(self, nll, skip_flag=None, stream=None):
        """After model.step (params still hold the sample; nll = its (B,) device losses): clip, L2, gradient noise
        on grads in place, then the module's updateOutput + accGradParameters into gradWeight (timit.lua:297-333).
        skip_flag as in Adadelta.step: nonzero (or the context's failure status set) when this runs on the device
        leaves grads, gradWeight and both counters untouched; gradnorm is still written."""
        if not (nll.is_cuda and nll.dtype == torch.float32 and nll.is_contiguous() and nll.numel() >= 1):
            raise ValueError("nll must be a contiguous float32 CUDA tensor of the minibatch's losses")
        args = (self.ctx.handle, self._st(stream), ctypes.byref(self.cfg), dptr(self.weight), dptr(self.params),
                dptr(self.grads), dptr(self.gradWeight), self.n, dptr(nll), nll.numel(), dptr(self.state),
                dptr(self.out))
        if skip_flag is None:
            check(lib.s2s_wnoise_backward(*args))
            return
        if not (skip_flag.is_cuda and skip_flag.dtype == torch.float32 and skip_flag.numel() >= 1):
            raise ValueError("skip_flag must be a float32 CUDA tensor")
        check(lib.s2s_wnoise_backward_flag(*args, dptr(skip_flag)))

    def mode(self, stream=None):
        """parameters <- Mode() (mu / weight) before evaluation or beam search (timit.lua:375-379)."""
        check(lib.s2s_wnoise_mode(self.ctx.handle, self._st(stream), ctypes.byref(self.cfg), dptr(self.weight),
                                  dptr(self.params), self.n))

    def set_steps(self, t_sample, t_gradnoise, stream=None):
        """Counters of a resumed run: the next sample() draws with t_sample + 1, the next noised backward() with
        t_gradnoise + 1 (gradnoise.t, timit.lua:92, 312)."""
        check(lib.s2s_wnoise_set_steps(self.ctx.handle, self._st(stream), dptr(self.state), int(t_sample),
                                       int(t_gradnoise)))

    def steps(self):
        """(t_sample, t_gradnoise) read back from the device (synchronises)."""
        t = self.state[:8].view(torch.int32).cpu()
        return int(t[0]) & 0xFFFFFFFF, int(t[1]) & 0xFFFFFFFF

    def state_dict(self):
        t_s, t_g = self.steps()
        return {"weight": self.weight.detach().clone(), "t_sample": t_s, "t_gradnoise": t_g,
                "sample_seed": int(self.cfg.sample_seed), "gradnoise_seed": int(self.cfg.gradnoise_seed)}

    def load_state_dict(self, sd):
        if sd["weight"].numel() != self.weight.numel():
            raise ValueError("state_dict's weight has another size (adaptive vs fixed, or another model)")
        self.weight.copy_(sd["weight"])
        self.cfg.sample_seed, self.cfg.gradnoise_seed = int(sd["sample_seed"]), int(sd["gradnoise_seed"])
        self.set_steps(sd["t_sample"], sd["t_gradnoise"])


class WeightNoise(_WeightNoiseBase):
    """nn.WeightNoise(parameters, sigma) (WeightNoise.lua; opt.weightnoise, timit.lua:190-195): weight (n) starts
    as the parameters, sample() sets parameters = weight + sigma * N(0, 1), backward() leaves gradWeight = the
    clipped / decayed / noised gradient and L = nll, mode() restores parameters = weight.  See _WeightNoiseBase
    for the loop and the three differences from the reference."""

    def __init__(self, model=None, sigma=1e-3, params=None, grads=None, maxnorm=1e20, weightDecay=0.0,
                 gradnoise_eta=0.0, gradnoise_gamma=0.55, gradnoise_seed=0x5EED, sample_seed=0x5A3D1E, ctx=None):
        super().__init__(False, 0.0, sigma, model, params, grads, maxnorm, weightDecay, gradnoise_eta,
                         gradnoise_gamma, gradnoise_seed, sample_seed, ctx)


class AdaptiveWeightNoise(_WeightNoiseBase):
    """nn.AdaptiveWeightNoise(parameters, lambda, sigma_init) (AdaptiveWeightNoise.lua; opt.adaweightnoise,
    opt.adalambda = 1/B, opt.adasigmainit, timit.lua:196-205): weight = [mu ; s] (2n), s = log sigma^2, starting
    at mu = parameters, s = log(sigma_init^2).  sample() sets parameters = mu + exp(s)^0.5 * N(0, 1);
    backward() computes alpha_mu, alpha_sigma2, KL and L = adalambda * KL + nll (:63-80) and gradWeight =
    [gradmu ; grads] (:82-104); mode() restores parameters = mu.  The sums behind alpha_* and KL are taken in
    double in a fixed order.  See _WeightNoiseBase for the loop and the three differences from the reference."""

    def __init__(self, model=None, adalambda=1.0, sigma_init=1.0, params=None, grads=None, maxnorm=1e20,
                 weightDecay=0.0, gradnoise_eta=0.0, gradnoise_gamma=0.55, gradnoise_seed=0x5EED,
                 sample_seed=0x5A3D1E, ctx=None):
        super().__init__(True, adalambda, sigma_init, model, params, grads, maxnorm, weightDecay, gradnoise_eta,
                         gradnoise_gamma, gradnoise_seed, sample_seed, ctx)

    @property
    def mu(self):
        return self.weight[:self.n]

    @property
    def s(self):
        return self.weight[self.n:]
