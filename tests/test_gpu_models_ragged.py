"""GPU: the conv + BiLSTM and VGG attention models on padded batches of variable-length utterances.

Every reference is the float64 oracle run per utterance on the utterance's own frames and labels (the reference
trainer's loop, timit/timit.lua:239-295 and :368-417, librispeech/train.lua:82-261); gradients are summed over the
utterances at scale 1/B.  Bar: max|gpu - ref| <= 1e-4 max|ref| per tensor.  Discrete decisions (ReLU, max pooling,
MonotonicAlignment) are the GPU's where the oracle's margin is within fp32 noise and must agree everywhere else, as
in tests/test_frontend.py; where a test cannot read the GPU's decisions (step_ragged runs several batches) the
case is chosen so that the oracle has no near tie at all, and asserts that.

1-2  the decoder alone with hybrid location-aware attention and frame lengths (per-step kernels; the timit.lua
     widths, where the dispatch may pick the XCD-local LSTM kernels): these pin kernel paths that had no test.
3-9  the model-level surface: step / forward with lengths, step_ragged, graph replay with DeviceLengths,
     Evaluate, refusals.
"""
import numpy as np
import pytest
import torch

import paths
from oracle import frontend_oracle as fo
from oracle import s2s_oracle as orc
from test_frontend import FLOOR_FACTOR, _load_lstm_attention, _timit_lstm_dec_case

pytestmark = pytest.mark.gpu
RTOL = 1e-4
MARGIN = 1e-5
_cache = {}


@pytest.fixture(scope="module")
def s2s():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import s2s_amd
    return s2s_amd


@pytest.fixture(scope="module")
def fe(s2s):
    from s2s_amd import frontend
    return frontend


def cu(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _np(t):
    return t.detach().cpu().double().numpy()


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def rel(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return float(np.abs(a - r).max() / max(np.abs(r).max(), 1e-30))


def check(errs, floors=None):
    """1e-4 per tensor; a tensor's bar rises only to FLOOR_FACTOR x the fp32 restatement's own error (floors)."""
    print({k: f"{v:.1e}" for k, v in errs.items()})
    floors = floors or {}
    bad = {k: f"{v:.2e}" for k, v in errs.items() if not v <= max(RTOL, FLOOR_FACTOR * floors.get(k, 0.0))}
    assert not bad, bad


def _onehot(labels, O):
    oh = np.zeros(labels.shape + (O,))
    np.put_along_axis(oh, labels[..., None].astype(np.int64), 1.0, axis=-1)
    return oh


# ------------------------------------------------------------------ 1-2: the decoder alone, hybrid + lengths

FLEN, TLEN = [24, 17, 16, 3, 1], [6, 1, 4, 6, 2]  # the 16-frame chunk edge, shorter than the filter, one frame


def _ragged_h(rng, B, L, A, lens, scale):
    """Real frames at `scale`; padding frames hold finite garbage at 3x that scale (masked, never read)."""
    h = rng.standard_normal((B, L, A)) * scale
    for b, Lb in enumerate(lens):
        h[b, Lb:] = rng.standard_normal((L - Lb, A)) * 3 * scale
    return _f32(h)


def _adopt_mono(cache, gind_b, Lb):
    """The GPU's MonotonicAlignment decisions where the statistic is within fp32 noise of 0; equal elsewhere."""
    a = cache["alpha"]
    prev = np.concatenate([np.zeros_like(a[:, :1]), a[:, :-1]], 1)
    stat = ((Lb - np.arange(Lb))[None, None, :] * (a - prev)).sum(-1)
    clear = np.abs(stat) > 1e-4
    assert np.array_equal(gind_b[clear], cache["mono_ind"][clear]), "MonotonicAlignment decisions differ"
    cache["mono_ind"] = gind_b


def _decoder_with_lengths(att, P, cfg, h, labels, flen, tlen, rng, grad_pairs, layers=None):
    """Run att on the padded batch with lengths; compare logp, alpha, dh and every parameter gradient with the oracle
    decoder run on each utterance's own frames and labels; exact zeros on the padding.  layers: the external
    decoder_mlp's oracle layers (None: the fused MaxoutMLP).  grad_pairs(G, mg) -> [(name, gpu tensor, ref)]."""
    B, L, T, O = h.shape[0], h.shape[1], labels.shape[1], cfg.outputDepth
    pen = cfg.penalty
    flen, tlen = np.asarray(flen), np.asarray(tlen)
    att.frame_lengths, att.label_lengths = flen, tlen
    hs = cu(h)
    with paths.decisions() as dec:
        logp = _np(att.forward([hs, cu(labels, torch.int32)]))
        alpha = _np(att.alpha())
        gind = _np(att.mono_ind())
        dlogp = _f32(rng.standard_normal(logp.shape))
        dlogp[np.arange(T)[None, :] >= tlen[:, None]] = 0.0  # nll_seed's dlogp on padding steps
        att.zeroGradParameters()
        dh = _np(att.backward([hs, None], cu(dlogp), 0.5)[0])
        torch.cuda.synchronize()
    att.frame_lengths = att.label_lengths = None
    print("decoder path:", {n: dec.get(n) for n in ("dec.fwd.path", "dec.bwd.path", "dec.var", "dec.res")})
    G = {k: np.zeros_like(v) for k, v in P.items()}
    mg = None if layers is None else [(np.zeros_like(Lr[1]), np.zeros_like(Lr[2])) if Lr[0] == "linear" else None
                                      for Lr in layers]
    dhr = np.zeros_like(h)
    lerr, aerr, lmax = 0.0, 0.0, 0.0
    lrefs = []
    for b in range(B):
        Lb, Tb = int(flen[b]), int(tlen[b])
        lref, cache = orc.attention_fwd(h[b:b + 1, :Lb], labels[b:b + 1, :Tb], P, cfg)
        if pen > 0:
            _adopt_mono(cache, gind[b:b + 1, :Tb], Lb)
        if layers is None:
            dhr[b:b + 1, :Lb] = orc.attention_bwd(P, cfg, cache, dlogp[b:b + 1, :Tb], G, 0.5)
        else:
            lref, mc = fo.mlp_fwd(cache["v"].reshape(Tb, -1), layers)
            lref = lref[None]
            dv = fo.mlp_bwd(layers, mc, dlogp[b, :Tb], mg, 0.5)
            dhr[b:b + 1, :Lb] = orc.attention_bwd(P, cfg, cache, None, G, 0.5, dmlp_in=dv.reshape(1, Tb, -1))
        lrefs.append(lref[0])
        lmax = max(lmax, np.abs(lref).max())
        aerr = max(aerr, np.abs(alpha[b, :Tb, :Lb] - cache["alpha"][0]).max())
    lerr = max(np.abs(logp[b, :int(tlen[b])] - lrefs[b]).max() for b in range(B)) / lmax
    errs = {"logp": lerr, "alpha (abs)": aerr, "dh": rel(dh, dhr)}
    errs.update({n: rel(_np(g), r) for n, g, r in grad_pairs(G, mg)})
    check(errs)
    assert (alpha[np.broadcast_to(np.arange(L)[None, None, :] >= flen[:, None, None], alpha.shape)] == 0).all()
    assert (dh[np.arange(L)[None, :] >= flen[:, None]] == 0).all()
    assert (gind[np.arange(T)[None, :] >= tlen[:, None]] == 0).all()
    return dec


@pytest.mark.parametrize("pen", [0.0, 0.3])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_hybrid_attention_lengths_per_step_kernels(s2s, cell, pen):
    """Attention(LSTM(32, 32) | GRU(32, 32), MaxoutMLP, Sc = 20, kW = 5, nF = 8, A = 32, O = 11) with frame lengths
    [24, 17, 16, 3, 1] and label lengths [6, 1, 4, 6, 2] of L = 24, T = 6: the location features of a padded batch
    (the convolution of alpha_{t-1} reads zeros past L_b, as the utterance alone reads its zero padding)."""
    S, A, Sc, O, M, Kw, kW, nF = 32, 32, 20, 11, 4, 3, 5, 8
    B, L, T = 5, 24, 6
    rng = np.random.default_rng(100 + (cell == "gru") + int(10 * pen))
    g = torch.Generator().manual_seed(5)
    lstm = cell == "lstm"
    rec = s2s.LSTM(S, S, False, g) if lstm else s2s.GRU(S, S, g)
    mlp = s2s.MaxoutMLP(S + A, M, Kw, O, g)
    att = s2s.Attention(rec, mlp, Sc, kW, nF, S, A, O, True, pen, generator=g).cuda()
    with torch.no_grad():
        att.own["hybU"].mul_(4.0)  # the location features visibly steer the scores
    cfg = orc.ModelConfig(inputFrameSize=8, hiddenFrameSize=16, outputFrameSize=A // 2, scoreDepth=Sc, stateDepth=S,
                          outputDepth=O, mlpDepth=M, maxoutWindow=Kw, numLayers=1, penalty=pen,
                          hybridAttendFilterSize=kW, hybridAttendFeatureMaps=nF, decoderLSTM=lstm)
    h = _ragged_h(rng, B, L, A, FLEN, 0.5)
    labels = rng.integers(0, O, (B, T)).astype(np.int32)
    att.forward([cu(h), cu(labels, torch.int32)])  # (binds the padded score channels before P is read)
    P = {n: _np(t) for n, t in att.own.items()}
    if lstm:
        P.update({"dec." + n: _np(t) for n, t in rec.named().items()})
    else:
        P.update({"dec.W" + q: _np(t) for q, t in zip("zrh", rec.weight)})
    P.update({n: _np(t) for n, t in zip(("Wm", "bm", "Wo", "bo"), mlp.weight)})

    def pairs(G, mg):
        out = [("d" + n, t, G[n]) for n, t in att.own_grad.items()]
        if lstm:
            out += [("ddec." + n, t, G["dec." + n]) for n, t in rec.named(grads=True).items()]
        else:
            out += [("ddec.W" + q, t, G["dec.W" + q]) for q, t in zip("zrh", rec.gradWeight)]
        return out + [("d" + n, t, G[n]) for n, t in zip(("Wm", "bm", "Wo", "bo"), mlp.gradWeight)]

    dec = _decoder_with_lengths(att, P, cfg, h, labels, FLEN, TLEN, rng, pairs)
    paths.took(dec, "dec.fwd.path", paths.STEPS)
    paths.took(dec, "dec.bwd.path", paths.STEPS)


@pytest.mark.parametrize("pen", [0.0, 0.3])
@pytest.mark.parametrize("mode", ["auto", "step"])
def test_hybrid_attention_lengths_timit_widths(s2s, fe, mode, pen):
    """The same contract at the timit/timit.lua:127-155 decoder's widths (LSTM(400, 400), A = 256, scoreDepth 150
    on 160 padded channels, kW = 5, 16 maps, external ReLU decoder_mlp): in auto mode the dispatch may take the
    XCD-local LSTM kernels (dec_xcd_lstm.inc) -- every chunk publishes its scores and alpha granules for all L frames
    whatever L_b is, so the padded batch waits on nothing that is not written -- and with the decoder mode forced
    to `step` the per-step kernels.  The log names the path each arm proved."""
    S, A, Sc, O, kW, nF = 400, 256, 150, 62, 5, 16
    B, L, T = 5, 24, 6
    rng = np.random.default_rng(7 + int(10 * pen))
    cfg, P = _timit_lstm_dec_case(rng, S, A, Sc, O, kW, nF)
    P = {k: _f32(v) for k, v in P.items()}
    cfg.penalty = pen
    mlp = fe.Sequential(fe.Linear(S + A, 2 * O), fe.ReLU(), fe.Linear(2 * O, O), fe.LogSoftMax())
    att, cell = _load_lstm_attention(s2s, fe, P, cfg, mlp)
    lins = [m for m in mlp.modules if isinstance(m, fe.Linear)]
    layers = [("linear", _np(lins[0].weight), _np(lins[0].bias)), ("relu",),
              ("linear", _np(lins[1].weight), _np(lins[1].bias)), ("logsoftmax",)]
    h = _ragged_h(rng, B, L, A, FLEN, 0.5)
    labels = rng.integers(0, O, (B, T)).astype(np.int32)

    def pairs(G, mg):
        out = [("d" + n, t, G[n]) for n, t in att.own_grad.items()]
        out += [("ddec." + n, t, G["dec." + n]) for n, t in cell.named(grads=True).items()]
        return out + [("dmlp0.W", lins[0].gradWeight, mg[0][0]), ("dmlp0.b", lins[0].gradBias, mg[0][1]),
                      ("dmlp2.W", lins[1].gradWeight, mg[2][0]), ("dmlp2.b", lins[1].gradBias, mg[2][1])]

    with paths.dec_mode(paths.MODE_STEP if mode == "step" else paths.MODE_AUTO):
        dec = _decoder_with_lengths(att, P, cfg, h, labels, FLEN, TLEN, rng, pairs, layers)
    if mode == "step":
        paths.took(dec, "dec.fwd.path", paths.STEPS)
        paths.took(dec, "dec.bwd.path", paths.STEPS)
    else:
        assert dec["dec.fwd.path"] == dec["dec.bwd.path"]


# ------------------------------------------------------------------ the two models at test widths

CONV_KW = dict(numPhonemes=11, hiddenFrameSize=32, outputFrameSize=16, stateDepth=32, scoreDepth=20)
VGG_KW = dict(outputFrameSize=128, hidden=128, scoreDepth=128, stateDepth=64, outputDepth=29, mlpDepth=8)


def _make_conv(s2s, seed=13, sharpen=False, cuda=True):
    m = s2s.ConvBiLSTMAttentionModel(20, generator=torch.Generator().manual_seed(seed), **CONV_KW)
    if cuda:
        m.cuda()
    if sharpen:
        with torch.no_grad():
            m.decoder.own["Wy"].mul_(3.0)
            m.decoder.own["we"].mul_(3.0)
            m.decoder.decoder_mlp.modules[2].weight.mul_(3.0)
    return m


def _make_vgg(s2s, seed=9, sharpen=False, cuda=True, **kw):
    kw = {**VGG_KW, **kw}
    Fq = kw.pop("Fq", 40)
    m = s2s.VGGAttentionModel(Fq, generator=torch.Generator().manual_seed(seed), **kw)
    if cuda:
        m.cuda()
    mods = m.encoder.seq.modules
    # conditioning, as tests/test_frontend.py::test_vgg_attention_model_step_matches_oracle: zero encoder biases
    # and a larger last layer give O(1) annotations that differ across frames
    with torch.no_grad():
        for mod in mods:
            if getattr(mod, "bias", None) is not None:
                mod.bias.zero_()
        [mod for mod in mods if type(mod).__name__ == "TemporalConvolution"][-1].weight.mul_(20.0)
        if sharpen:
            m.decoder.own["Wy"].mul_(3.0)
            m.decoder.own["we"].mul_(3.0)
            m.decoder.decoder_mlp.modules[3].weight.mul_(3.0)
    return m


def _conv_params(fe, model):
    enc, dec = model.encoder, model.decoder
    c = {"convs": [m for m in enc.convlayer.modules if isinstance(m, fe.TemporalConvolution)],
         "pools": [m for m in enc.convlayer.modules if isinstance(m, fe.TemporalMaxPooling)],
         "lins": [m for m in dec.decoder_mlp.modules if isinstance(m, fe.Linear)]}
    dec._sync_pad()
    P = {}
    for l, m in enumerate(c["convs"]):
        P[f"conv{l}.W"], P[f"conv{l}.b"] = _np(m.weight), _np(m.bias)
    for pre, cell in zip(("f.", "b."), enc.rnn.cells):
        for k, v in cell.named().items():
            P[pre + k] = _np(v)
    Pd = {n: _np(t) for n, t in dec.own.items()}
    for n, t in dec.decoder_recurrent.named().items():
        Pd["dec." + n] = _np(t)
    S, A, O = dec.stateDepth, dec.annotationDepth, dec.outputDepth
    for name, shp in (("Wm", (3, S + A)), ("bm", (3,)), ("Wo", (O, 1)), ("bo", (O,))):
        Pd[name] = np.zeros(shp)
    c["cfg"] = orc.ModelConfig(inputFrameSize=8, hiddenFrameSize=16, outputFrameSize=A // 2, scoreDepth=dec.scoreDepth,
                               stateDepth=S, outputDepth=O, mlpDepth=1, maxoutWindow=3, numLayers=1,
                               hybridAttendFilterSize=5, hybridAttendFeatureMaps=16, decoderLSTM=True)
    lins = c["lins"]
    c["layers"] = [("linear", _np(lins[0].weight), _np(lins[0].bias)), ("relu",),
                   ("linear", _np(lins[1].weight), _np(lins[1].bias)), ("logsoftmax",)]
    c["P"], c["Pd"] = P, Pd
    return c


def _conv_grad_pairs(model, c, Ge, Gd, mg):
    enc, dec = model.encoder, model.decoder
    pairs = []
    for l, m in enumerate(c["convs"]):
        pairs += [(f"dconv{l}.W", m.gradWeight, Ge[f"conv{l}.W"]), (f"dconv{l}.b", m.gradBias, Ge[f"conv{l}.b"])]
    for pre, cell in zip(("f.", "b."), enc.rnn.cells):
        pairs += [(f"d{pre}{k}", g, Ge[pre + k]) for k, g in cell.named(grads=True).items()]
    pairs += [("d" + n, g, Gd[n]) for n, g in dec.own_grad.items()]
    pairs += [("ddec." + n, g, Gd["dec." + n]) for n, g in dec.decoder_recurrent.named(grads=True).items()]
    lins = c["lins"]
    return pairs + [("dmlp0.W", lins[0].gradWeight, mg[0][0]), ("dmlp0.b", lins[0].gradBias, mg[0][1]),
                    ("dmlp2.W", lins[1].gradWeight, mg[2][0]), ("dmlp2.b", lins[1].gradBias, mg[2][1])]


def _conv_decisions(c, ccache, b=None):
    """The conv stack's ReLU and max-pooling decisions of one utterance.  b = its row in the GPU's last batch: the
    GPU's decisions are adopted inside the near-tie band (MARGIN x max|u|) and must agree outside it.  b = None
    (nothing to adopt from): the oracle itself must have no near tie."""
    for l, (tc, tp) in enumerate(zip(c["convs"], c["pools"])):
        h, u, idx, Lr = ccache[l]
        scale = np.abs(u).max()
        r = np.maximum(u, 0.0)[:, :2 * idx.shape[1]].reshape(1, idx.shape[1], 2, -1)
        gap = np.abs(r[:, :, 0] - r[:, :, 1])
        clear, clear_p = np.abs(u) > MARGIN * scale, (gap > MARGIN * scale) | (r.max(2) <= 0)
        if b is None:
            assert clear.all() and clear_p.all(), f"layer {l}: the oracle has a near tie; choose another seed"
            continue
        gmask = _np(tc.output)[b:b + 1, :u.shape[1]] > 0
        assert np.array_equal(gmask[clear], (u > 0)[clear]), f"layer {l}: ReLU decisions differ off the near-tie band"
        gidx = tp.indices.cpu().numpy()[b:b + 1, :idx.shape[1]].astype(idx.dtype)
        live = clear_p & (r.max(2) > 0)  # (a window of two zeros routes its gradient into a closed ReLU either way)
        assert np.array_equal(gidx[live], idx[live]), f"layer {l}: max-pooling decisions differ off the band"
        ccache[l] = (h, np.where(gmask, 1.0, -1.0), gidx, Lr)


def _conv_reference(c, xs, ys, scale, rows=None, backward=True):
    """The oracle per utterance on its own frames (fp32-rounded, as the GPU sees them): (nll list, logp list,
    annotations list, encoder grads, decoder grads, mlp grads), gradients summed at `scale`."""
    P, Pd, cfg, layers = c["P"], c["Pd"], c["cfg"], c["layers"]
    O = cfg.outputDepth
    Ge = {k: np.zeros_like(v) for k, v in P.items()}
    Gd = {k: np.zeros_like(v) for k, v in Pd.items()}
    mg = [(np.zeros_like(Lr[1]), np.zeros_like(Lr[2])) if Lr[0] == "linear" else None for Lr in layers]
    nll, logps, hs = [], [], []
    for i, (x, y) in enumerate(zip(xs, ys)):
        h, ecache = fo.conv_bilstm_fwd(x[None], P)
        _, acache = orc.attention_fwd(h, y[None], Pd, cfg)
        lref, mc = fo.mlp_fwd(acache["v"].reshape(len(y), -1), layers)
        oh = _onehot(y, O)
        nll.append(-(oh * lref).sum())
        logps.append(lref)
        hs.append(h[0])
        if backward:
            dv = fo.mlp_bwd(layers, mc, -oh, mg, scale)
            dh = orc.attention_bwd(Pd, cfg, acache, None, Gd, scale, dmlp_in=dv.reshape(1, len(y), -1))
            _conv_decisions(c, ecache[1], None if rows is None else rows[i])
            fo.conv_bilstm_bwd(P, ecache, dh, Ge, scale)
    return nll, logps, hs, Ge, Gd, mg


def _vgg_params(fe, model):
    enc_mods, dec = model.encoder.seq.modules, model.decoder
    c = {"sconvs": [m for m in enc_mods if isinstance(m, fe.SpatialConvolutionMM)],
         "tconvs": [m for m in enc_mods if isinstance(m, fe.TemporalConvolution)]}
    P = {}
    for l, m in enumerate(c["sconvs"]):
        P[f"vgg{l}.W"], P[f"vgg{l}.b"] = _np(m.weight), _np(m.bias)
    for l, m in enumerate(c["tconvs"]):
        P[f"lin{l}.W"], P[f"lin{l}.b"] = _np(m.weight), _np(m.bias)
    c["names"] = ("V", "Ws", "bs", "we", "Wy", "by", "Wc", "bc", "Wd", "bd", "dec.Wz", "dec.Wr", "dec.Wh")
    dec._sync_pad()
    for n, t in zip(c["names"], dec._tensors(False)[:13]):
        P[n] = _np(t)
    layers = []
    for m in dec.decoder_mlp.modules:
        if isinstance(m, fe.Maxout):
            layers.append(("maxout", _np(m.linear.weight), _np(m.linear.bias), m.window))
        elif isinstance(m, fe.Linear):
            layers.append(("linear", _np(m.weight), _np(m.bias)))
        else:
            layers.append(("logsoftmax",))
    c["mlp_mods"] = [m for m in dec.decoder_mlp.modules if not isinstance(m, fe.LogSoftMax)]
    c["cfg"] = orc.ModelConfig(inputFrameSize=8, hiddenFrameSize=16, outputFrameSize=dec.annotationDepth // 2,
                               scoreDepth=dec.scoreDepth, stateDepth=dec.stateDepth, outputDepth=dec.outputDepth,
                               mlpDepth=dec.decoder_mlp.modules[0].outputDim, maxoutWindow=7, numLayers=1)
    c["P"], c["layers"] = P, layers
    return c


def _vgg_grad_pairs(fe, model, c, G, mg):
    pairs = []
    for l, m in enumerate(c["sconvs"]):
        pairs += [(f"dvgg{l}.W", m.gradWeight, G[f"vgg{l}.W"]), (f"dvgg{l}.b", m.gradBias, G[f"vgg{l}.b"])]
    for l, m in enumerate(c["tconvs"]):
        pairs += [(f"dlin{l}.W", m.gradWeight, G[f"lin{l}.W"]), (f"dlin{l}.b", m.gradBias, G[f"lin{l}.b"])]
    pairs += [("d" + n, g, G[n]) for n, g in zip(c["names"], model.decoder._tensors(True)[:13])]
    for i, (m, g) in enumerate(zip(c["mlp_mods"], [g for g in mg if g is not None])):
        lin = m.linear if isinstance(m, fe.Maxout) else m
        pairs += [(f"dmlp{i}.W", lin.gradWeight, g[0]), (f"dmlp{i}.b", lin.gradBias, g[1])]
    return pairs


def _vgg_reference(c, xs, ys, scale, dtype=np.float64):
    """fo.vgg_model_step per utterance (x (3, L_b, F), its own labels), gradients summed at `scale`."""
    P = {k: v.astype(dtype) for k, v in c["P"].items()}
    layers = [tuple(a.astype(dtype) if isinstance(a, np.ndarray) else a for a in Lr) for Lr in c["layers"]]
    G, mg, nll, logps = None, None, [], []
    for x, y in zip(xs, ys):
        n, lp, Gb, mgb = fo.vgg_model_step(x[None].astype(dtype), y[None], P, layers, c["cfg"])
        nll.append(n[0])
        logps.append(lp[0])
        if G is None:
            G = {k: scale * v for k, v in Gb.items()}
            mg = [None if g is None else (scale * g[0], scale * g[1]) for g in mgb]
        else:
            for k, v in Gb.items():
                G[k] += scale * v
            mg = [None if g is None else (g[0] + scale * gb[0], g[1] + scale * gb[1]) for g, gb in zip(mg, mgb)]
    return nll, logps, G, mg


def _pad(xs, ys, axis, garbage=None):
    """Zero-padded (or garbage-padded: finite values at 3x scale on the padding frames) batch of the utterances."""
    Ls, Ts = [x.shape[axis] for x in xs], [len(y) for y in ys]
    shape = list(xs[0].shape)
    shape[axis] = max(Ls)
    x = np.zeros([len(xs)] + shape)
    if garbage is not None:
        x = _f32(garbage.standard_normal(x.shape) * 3 * np.abs(xs[0]).std())
    y = np.zeros((len(xs), max(Ts)), np.int32)
    for b, (xb, yb) in enumerate(zip(xs, ys)):
        sl = [b] + [slice(None)] * len(shape)
        sl[axis + 1] = slice(0, Ls[b])
        x[tuple(sl)] = xb
        y[b, :Ts[b]] = yb
    return x, y, Ls, Ts


def _snapshot(model, nll, logp):
    torch.cuda.synchronize()
    return [nll.clone(), logp.clone()] + [g.clone() for g in model.parameters()[1]]


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _utterances(rng, Ls, Ts, O, shape, scale=1.0, eos=None):
    xs = [_f32(rng.standard_normal(shape(L)) * scale) for L in Ls]
    ys = []
    for T in Ts:
        y = rng.integers(0, O - 1 if eos is not None else O, T).astype(np.int32)
        if eos is not None:
            y[-1] = eos
        ys.append(y)
    return xs, ys


# ------------------------------------------------------------------ 3: full lengths = no lengths, bit for bit

@pytest.mark.parametrize("which", ["conv", "vgg"])
def test_full_lengths_equal_no_lengths_bitwise(s2s, which):
    rng = np.random.default_rng(3)
    if which == "conv":
        model, B, L, T, O = _make_conv(s2s), 3, 60, 5, 11
        x = cu(rng.standard_normal((B, L, 20)))
    else:
        model, B, L, T, O = _make_vgg(s2s), 2, 40, 6, 29
        x = cu(rng.standard_normal((B, 3, L, 40)) * 10)
    labels = cu(rng.integers(0, O, (B, T)), torch.int32)
    model.zeroGradParameters()
    a = _snapshot(model, *model.step(x, labels))
    model.zeroGradParameters()
    b = _snapshot(model, *model.step(x, labels, frame_lengths=[L] * B, label_lengths=[T] * B))
    assert _same(a, b)
    assert model.decoder.frame_lengths is None and model.decoder.label_lengths is None  # restored
    if which == "conv":
        assert model.encoder.rnn.lengths is None


# ------------------------------------------------------------------ 4-5: step with lengths

def test_conv_bilstm_model_step_with_lengths(s2s, fe):
    """B = 4, raw frames [60, 47, 33, 22] -> L' = [5, 4, 2, 1], labels [5, 3, 4, 1], against the per-utterance loop of
    fo.conv_bilstm_fwd / orc.attention_fwd / fo.mlp_fwd and their backwards; then the same step with garbage on the
    padding frames of x, which must change no bit of any output or gradient (the front-end needs no mask)."""
    rng = np.random.default_rng(13)
    model = _make_conv(s2s)
    c = _conv_params(fe, model)
    Ls, Ts, O = [60, 47, 33, 22], [5, 3, 4, 1], 11
    assert model.encoder.out_lengths(Ls) == [5, 4, 2, 1]
    xs, ys = _utterances(rng, Ls, Ts, O, lambda L: (L, 20))
    x, y, _, _ = _pad(xs, ys, 0)
    model.zeroGradParameters()
    nll, logp = model.step(cu(x), cu(y, torch.int32), frame_lengths=Ls, label_lengths=Ts)
    zero = _snapshot(model, nll, logp)
    nll_r, logp_r, _, Ge, Gd, mg = _conv_reference(c, xs, ys, 1.0 / 4, rows=range(4))
    lmax = max(np.abs(l).max() for l in logp_r)
    errs = {"logp": max(np.abs(_np(logp)[b, :Ts[b]] - logp_r[b]).max() for b in range(4)) / lmax,
            "nll": rel(_np(nll), nll_r)}
    errs.update({n: rel(_np(g), r) for n, g, r in _conv_grad_pairs(model, c, Ge, Gd, mg)})
    check(errs)
    xg, _, _, _ = _pad(xs, ys, 0, garbage=rng)
    assert np.abs(xg[3, 22:]).min() > 0
    model.zeroGradParameters()
    garb = _snapshot(model, *model.step(cu(xg), cu(y, torch.int32), frame_lengths=Ls, label_lengths=Ts))
    assert _same(zero, garb), "padding frames of x leak into the step"


def test_vgg_model_step_with_lengths(s2s, fe):
    """B = 3, raw frames [40, 29, 10] -> L' = [16, 10, 1], labels [4, 2, 3], against fo.vgg_model_step per utterance;
    then the garbage-padding run, bitwise equal.  A tensor's bar rises above 1e-4 only to FLOOR_FACTOR x the error
    of the oracle's own fp32 restatement on these inputs (tests/test_frontend.py)."""
    rng = np.random.default_rng(9)
    model = _make_vgg(s2s)
    c = _vgg_params(fe, model)
    Ls, Ts, O = [40, 29, 10], [4, 2, 3], 29
    assert model.encoder.out_lengths(Ls) == [16, 10, 1]
    xs, ys = _utterances(rng, Ls, Ts, O, lambda L: (3, L, 40), 10.0, eos=O - 1)
    x, y, _, _ = _pad(xs, ys, 1)
    model.zeroGradParameters()
    nll, logp = model.step(cu(x), cu(y, torch.int32), frame_lengths=Ls, label_lengths=Ts)
    zero = _snapshot(model, nll, logp)
    nll_r, logp_r, G, mg = _vgg_reference(c, xs, ys, 1.0 / 3)
    _, _, G32, mg32 = _vgg_reference(c, xs, ys, 1.0 / 3, np.float32)
    lmax = max(np.abs(l).max() for l in logp_r)
    errs = {"logp": max(np.abs(_np(logp)[b, :Ts[b]] - logp_r[b]).max() for b in range(3)) / lmax,
            "nll": rel(_np(nll), nll_r)}
    pairs = _vgg_grad_pairs(fe, model, c, G, mg)
    errs.update({n: rel(_np(g), r) for n, g, r in pairs})
    floors = {n: rel(r32, r) for (n, _, r), (_, _, r32) in zip(pairs, _vgg_grad_pairs(fe, model, c, G32, mg32))}
    uncapped = {n: f"{v:.1e}" for n, v in floors.items() if not v <= 1e-3}
    assert not uncapped, uncapped  # (a floor above 1e-3 would mean the case itself is unjudgeable)
    check(errs, floors)
    xg, _, _, _ = _pad(xs, ys, 1, garbage=rng)
    model.zeroGradParameters()
    garb = _snapshot(model, *model.step(cu(xg), cu(y, torch.int32), frame_lengths=Ls, label_lengths=Ts))
    assert _same(zero, garb), "padding frames of x leak into the step"


# ------------------------------------------------------------------ 6: step_ragged and forward

RAGGED_CONV_SEED = 20  # chosen on the CPU: the float64 oracle has no ReLU / pooling near tie on these utterances


def test_conv_bilstm_step_ragged_and_forward(s2s, fe):
    """6 utterances in batches of at most 4 (sorted by length: the input order is permuted) equal the per-utterance
    oracle sum at scale 1/6; forward() on a padded batch is bitwise the step's logp and nll."""
    rng = np.random.default_rng(RAGGED_CONV_SEED)
    model = _make_conv(s2s)
    c = _conv_params(fe, model)
    Ls, Ts, O = [33, 60, 22, 47, 51, 29], [4, 5, 1, 3, 2, 5], 11
    xs, ys = _utterances(rng, Ls, Ts, O, lambda L: (L, 20))
    nll, logps = model.step_ragged([cu(x) for x in xs], [cu(y, torch.int32) for y in ys], max_batch=4)
    torch.cuda.synchronize()
    nll_r, logp_r, _, Ge, Gd, mg = _conv_reference(c, xs, ys, 1.0 / 6)
    lmax = max(np.abs(l).max() for l in logp_r)
    assert [tuple(l.shape) for l in logps] == [(T, O) for T in Ts]
    errs = {"logp": max(np.abs(_np(logps[b]) - logp_r[b]).max() for b in range(6)) / lmax, "nll": rel(_np(nll), nll_r)}
    errs.update({n: rel(_np(g), r) for n, g, r in _conv_grad_pairs(model, c, Ge, Gd, mg)})
    check(errs)
    # length_multiple pads the same batches further (47 -> 48, 60 -> 64 frames) and graph=True replays each padded
    # shape from a capture: the same per-utterance sums, up to the fp32 summation order of the longer products
    nll2, logps2 = model.step_ragged([cu(x) for x in xs], [cu(y, torch.int32) for y in ys], max_batch=4, graph=True,
                                     length_multiple=8)
    torch.cuda.synchronize()
    assert sorted(model._ragged_bufs) == [(2, 64, 8), (4, 48, 8)]
    errs = {"logp": max(np.abs(_np(logps2[b]) - logp_r[b]).max() for b in range(6)) / lmax,
            "nll": rel(_np(nll2), nll_r)}
    errs.update({n: rel(_np(g), r) for n, g, r in _conv_grad_pairs(model, c, Ge, Gd, mg)})
    check(errs)
    x, y, L4, T4 = _pad(xs[:4], ys[:4], 0)
    model.zeroGradParameters()
    st = _snapshot(model, *model.step(cu(x), cu(y, torch.int32), frame_lengths=L4, label_lengths=T4))
    before = [g.clone() for g in model.parameters()[1]]
    n_f, l_f = model.forward(cu(x), cu(y, torch.int32), frame_lengths=L4, label_lengths=T4)
    torch.cuda.synchronize()
    assert torch.equal(n_f, st[0]) and torch.equal(l_f, st[1])
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()[1]))  # forward touches no gradient
    assert model.train


def test_vgg_step_ragged_and_forward(s2s, fe):
    rng = np.random.default_rng(10)
    model = _make_vgg(s2s)
    c = _vgg_params(fe, model)
    Ls, Ts, O = [29, 40, 10, 17, 36, 12], [4, 5, 1, 3, 2, 5], 29
    xs, ys = _utterances(rng, Ls, Ts, O, lambda L: (3, L, 40), 10.0, eos=O - 1)
    nll, logps = model.step_ragged([cu(x) for x in xs], [cu(y, torch.int32) for y in ys], max_batch=4)
    torch.cuda.synchronize()
    nll_r, logp_r, G, mg = _vgg_reference(c, xs, ys, 1.0 / 6)
    _, _, G32, mg32 = _vgg_reference(c, xs, ys, 1.0 / 6, np.float32)
    lmax = max(np.abs(l).max() for l in logp_r)
    errs = {"logp": max(np.abs(_np(logps[b]) - logp_r[b]).max() for b in range(6)) / lmax, "nll": rel(_np(nll), nll_r)}
    pairs = _vgg_grad_pairs(fe, model, c, G, mg)
    errs.update({n: rel(_np(g), r) for n, g, r in pairs})
    floors = {n: rel(r32, r) for (n, _, r), (_, _, r32) in zip(pairs, _vgg_grad_pairs(fe, model, c, G32, mg32))}
    assert all(v <= 1e-3 for v in floors.values()), floors
    check(errs, floors)
    x, y, L4, T4 = _pad(xs[:4], ys[:4], 1)
    model.zeroGradParameters()
    st = _snapshot(model, *model.step(cu(x), cu(y, torch.int32), frame_lengths=L4, label_lengths=T4))
    n_f, l_f = model.forward(cu(x), cu(y, torch.int32), frame_lengths=L4, label_lengths=T4)
    torch.cuda.synchronize()
    assert torch.equal(n_f, st[0]) and torch.equal(l_f, st[1])


# ------------------------------------------------------------------ 7: graph replay with DeviceLengths

@pytest.mark.parametrize("which", ["conv", "vgg"])
def test_graph_step_reads_lengths_at_replay(s2s, which):
    """graph_step with DeviceLengths is bitwise the eager step with the same lengths; then x, labels and both lengths
    are refilled in place from a second batch of the same padded shape (PackedUtterances.batch(out=...)) and the
    SAME capture replayed: bitwise that batch's eager step."""
    from s2s_amd.data import PackedUtterances
    rng = np.random.default_rng(17)
    if which == "conv":
        make, O, shape, Ls = (lambda: _make_conv(s2s)), 11, (lambda L: (L, 20)), [60, 47, 33, 22, 64, 25, 58, 40]
    else:
        make, O, shape, Ls = (lambda: _make_vgg(s2s)), 29, (lambda L: (3, L, 40)), [40, 29, 10, 33, 21, 38, 12, 40]
    Ts = [5, 3, 4, 1, 2, 6, 6, 3]
    xs, ys = _utterances(rng, Ls, Ts, O, shape, 10.0 if which == "vgg" else 1.0)
    pk = PackedUtterances(xs, ys)
    eager, graphed = make(), make()
    Lmax, Tmax = 64, 6
    bt = pk.batch([0, 1, 2, 3], Lmax, Tmax)
    for it, idx in enumerate(([0, 1, 2, 3], [0, 1, 2, 3], [4, 5, 6, 7])):
        if it == 2:
            assert pk.batch(idx, out=bt)[0] is bt[0]
        x, y, fl, tl = bt[:4]
        nll_g, logp_g = graphed.graph_step(x, y, None, False, fl, tl)
        eager.zeroGradParameters()
        nll_e, logp_e = eager.step(x, y, frame_lengths=fl, label_lengths=tl)
        torch.cuda.synchronize()
        assert torch.equal(logp_e, logp_g) and torch.equal(nll_e, nll_g), it
        for i, (ge, gg) in enumerate(zip(eager.parameters()[1], graphed.parameters()[1])):
            assert torch.equal(ge, gg), (it, i)
    assert len(graphed._graphs) == 1
    # and the replayed values are that batch's, not the captured one's: the eager step on a fresh padded copy
    x2, y2, L2, T2 = _pad(xs[4:], ys[4:], 0 if which == "conv" else 1)
    xp = np.zeros((4,) + tuple(bt[0].shape[1:]))
    xp[..., :x2.shape[-2], :] = x2
    yp = np.zeros((4, Tmax), np.int32)
    yp[:, :y2.shape[1]] = y2
    eager.zeroGradParameters()
    nll_l, logp_l = eager.step(cu(xp), cu(yp, torch.int32), frame_lengths=L2, label_lengths=T2)
    torch.cuda.synchronize()
    assert torch.equal(nll_l, nll_g) and torch.equal(logp_l, logp_g)
    with pytest.raises(ValueError):
        graphed.graph_step(x, y, None, False, Ls[:4], Ts[:4])  # host lists cannot be read at replay time


# ------------------------------------------------------------------ 8: Evaluate

EVAL_CONV_SEED, EVAL_VGG_SEED = 2, 65  # weight seeds chosen on the CPU (the assertions in _eval_reference hold)
EVAL_CONV_L, EVAL_VGG_L = [44, 22, 57, 38, 60, 41, 50], [25, 10, 40, 13, 36, 18, 29]
EVAL_T = [4, 2, 6, 3, 5, 3, 4]


def _eval_reference(kind, c, xs, ys, eos, K, factor):
    """Per utterance: the oracle's forward (nll, teacher-forced argmax), beam search on its own annotations with its
    own limit factor x L_b, in float64 and again in float32 -- the two must agree on every prediction and every
    argmax, so the case has no near tie of its own and any disagreement of the GPU is the GPU's."""
    out = {}
    for dtype in (np.float64, np.float32):
        res = []
        if kind == "conv":
            P = {k: v.astype(dtype) for k, v in c["P"].items()}
            Pd = {k: v.astype(dtype) for k, v in c["Pd"].items()}
        else:
            P = Pd = {k: v.astype(dtype) for k, v in c["P"].items()}
        layers = [tuple(a.astype(dtype) if isinstance(a, np.ndarray) else a for a in Lr) for Lr in c["layers"]]
        ext = lambda v: fo.mlp_fwd(v[None], layers)[0][0]  # noqa: E731
        Pb = dict(Pd)
        cfg = c["cfg"]
        S, A, M, k, O = cfg.stateDepth, cfg.annotationDepth, cfg.mlpDepth, cfg.maxoutWindow, cfg.outputDepth
        for name, shp in (("Wm", (M * k, S + A)), ("bm", (M * k,)), ("Wo", (O, M)), ("bo", (O,))):
            Pb.setdefault(name, np.zeros(shp, dtype))
        for x, y in zip(xs, ys):
            xd = x[None].astype(dtype)
            h = fo.conv_bilstm_fwd(xd, P)[0] if kind == "conv" else fo.vgg_fwd(xd, P)[0]
            _, acache = orc.attention_fwd(h, y[None], Pb, cfg)
            logp = fo.mlp_fwd(acache["v"].reshape(len(y), -1), layers)[0]
            Lraw = x.shape[0] if kind == "conv" else x.shape[1]
            seq, score = orc.beam_search(h[0], Pb, cfg, eos, K, maxseqlength=factor * Lraw, mlp=ext)
            res.append(dict(nll=float(-logp[np.arange(len(y)), y].sum()), argmax=logp.argmax(1).tolist(),
                            correct=int((logp.argmax(1) == y).sum()), h=h[0], seq=[int(t) for t in seq],
                            score=float(score)))
        out[dtype] = (res, Pb, ext)
    r64, r32 = out[np.float64][0], out[np.float32][0]
    assert [r["seq"] for r in r64] == [r["seq"] for r in r32], "fp32 and fp64 oracle predictions differ: another seed"
    assert [r["argmax"] for r in r64] == [r["argmax"] for r in r32], "fp32 and fp64 oracle argmax differ: another seed"
    return out[np.float64]


def _rescore(hb, seq, P, cfg, mlp):
    st, Vh, tot, y = orc.decoder_zero_state(hb.shape[0], cfg.stateDepth), hb @ P["V"].T, 0.0, -1
    for tok in seq:
        lp, st = orc.decoder_step(hb, Vh, st, y, P, cfg, mlp)
        tot, y = tot + lp[tok], tok
    return tot


def _eval_case(s2s, fe, kind, cuda=True, seed=None):
    """Shared by both token_map arms; computed once.  (cuda=False, seed: the CPU-side choice of the weight seed.)"""
    if kind in _cache and seed is None:
        return _cache[kind]
    rng = np.random.default_rng(31)
    if kind == "conv":
        model = _make_conv(s2s, seed or EVAL_CONV_SEED, sharpen=True, cuda=cuda)
        c = _conv_params(fe, model)
        O, Ls, shape, scale, factor = 11, EVAL_CONV_L, (lambda L: (L, 20)), 1.0, 1
    else:
        model = _make_vgg(s2s, seed or EVAL_VGG_SEED, sharpen=True, cuda=cuda, Fq=16, outputFrameSize=32, hidden=32,
                          scoreDepth=32, stateDepth=32, outputDepth=11, mlpDepth=4)
        c = _vgg_params(fe, model)
        O, Ls, shape, scale, factor = 11, EVAL_VGG_L, (lambda L: (3, L, 16)), 10.0, 2
    eos = O - 1
    xs, ys = _utterances(rng, Ls, EVAL_T, O, shape, scale, eos=eos)
    ref, Pb, ext = _eval_reference(kind, c, xs, ys, eos, 5, factor)
    _cache[kind] = (model, c, xs, ys, eos, ref, Pb, ext, factor)
    return _cache[kind]


@pytest.mark.parametrize("token_map", [False, True])
@pytest.mark.parametrize("kind", ["conv", "vgg"])
def test_evaluate_matches_the_oracle(s2s, fe, kind, token_map):
    """7 utterances, K = 5, batches of at most 4: numCorrect and distances exact, nll to 1e-4, predictions under the
    near-tie rule of tests/test_gpu_evaluate.py::_check_ragged (at most one differing prediction, and only when the
    oracle rescoring of it ties the oracle's best to 1e-4).  The conv model's raw lengths 38, 41 and 44 share one L'
    (3) and land in one batch: they must be searched as one group of 3.  A second run with garbage on the padding
    frames of every assembled batch returns the same bits."""
    from s2s_amd.data import PackedUtterances
    model, c, xs, ys, eos, ref, Pb, ext, factor = _eval_case(s2s, fe, kind)
    cfg, N = c["cfg"], len(xs)
    tmap = (np.arange(cfg.outputDepth) // 2) if token_map else None
    acc, nll, per, preds = model.Evaluate([cu(x) for x in xs], [torch.tensor(y) for y in ys], K=5, max_batch=4,
                                          token_map=tmap)
    det, groups = model.eval_detail, list(model.eval_groups)
    assert det["numCorrect"] == [r["correct"] for r in ref]
    assert acc == sum(r["correct"] for r in ref) / sum(len(y) for y in ys)
    for i, r in enumerate(ref):
        assert abs(det["nll"][i] - r["nll"]) <= RTOL * abs(r["nll"]), (i, det["nll"][i], r["nll"])
    assert nll == sum(det["nll"]) / N
    agree, pers = 0, []
    for i, r in enumerate(ref):
        seq = preds[i].tolist()
        Lraw = xs[i].shape[0 if kind == "conv" else 1]
        assert seq[-1] == eos or len(seq) == factor * Lraw + 1
        mine = _rescore(r["h"], seq, Pb, cfg, ext)
        print(f"utterance {i}: score {det['score'][i]:.6f}, oracle rescoring {mine:.6f}, oracle best {r['score']:.6f}")
        assert abs(mine - det["score"][i]) <= RTOL * max(1.0, abs(mine)), (i, mine, det["score"][i])
        if seq == r["seq"]:
            agree += 1
        else:
            assert abs(mine - r["score"]) <= RTOL * max(1.0, abs(r["score"])), (i, seq, r["seq"], mine, r["score"])
        a, b = (seq, ys[i].tolist()) if tmap is None else ([int(tmap[t]) for t in seq], [int(tmap[t]) for t in ys[i]])
        dist = orc.wagner_fischer(a, b)
        assert det["dist"][i] == dist, (i, det["dist"][i], dist)
        pers.append(dist / len(ys[i]))
    assert agree >= N - 1
    assert per == sum(pers) / N
    assert model.train
    if kind == "conv":
        # sorted by raw length: [22, 38, 41, 44] | [50, 57, 60] -> L' [1, 3, 3, 3] | [4, 5, 5]
        assert groups == [(1, [0]), (3, [1, 2, 3]), (4, [0]), (5, [1, 2])], groups
    else:
        assert groups == [(None, [0, 1, 2, 3]), (None, [0, 1, 2])], groups

    class GarbagePadding(PackedUtterances):
        def batch(self, idx, Lmax=None, Tmax=None, out=None):
            bt = super().batch(idx, Lmax, Tmax, out)
            g = torch.Generator(device="cuda").manual_seed(1)
            for j, L in enumerate(bt[4]):
                pad = bt[0][j, L:] if kind == "conv" else bt[0][j, :, L:]
                pad.copy_(torch.randn(pad.shape, generator=g, device="cuda") * 30)
            return bt

    first = (acc, nll, per, [p.tolist() for p in preds], dict(det))
    acc2, nll2, per2, preds2 = model.Evaluate(GarbagePadding(xs, ys), None, K=5, max_batch=4, token_map=tmap)
    assert (acc2, nll2, per2, [p.tolist() for p in preds2], model.eval_detail) == first


# ------------------------------------------------------------------ 9: refusals

def test_refusals(s2s):
    from s2s_amd.nn import S2SArgumentError
    conv, vgg = _make_conv(s2s), _make_vgg(s2s, Fq=16, outputFrameSize=32, hidden=32, scoreDepth=32, stateDepth=32,
                                           outputDepth=11, mlpDepth=4)
    x, y = torch.zeros((2, 60, 20), device="cuda"), torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(S2SArgumentError, match="22"):
        conv.step(x, y, frame_lengths=[60, 21], label_lengths=[3, 3])
    with pytest.raises(S2SArgumentError):
        conv.step(x, y, frame_lengths=[60, 30, 30], label_lengths=[3, 3])
    with pytest.raises(S2SArgumentError):
        conv.forward(x, y, frame_lengths=[60, 30], label_lengths=[3])
    with pytest.raises(S2SArgumentError):
        conv.step(x, y, frame_lengths=[61, 30], label_lengths=[3, 3])
    with pytest.raises(S2SArgumentError):
        conv.step(x, y, frame_lengths=[60, 30], label_lengths=[3, 4])
    xv = torch.zeros((2, 3, 20, 16), device="cuda")
    with pytest.raises(S2SArgumentError, match="10"):
        vgg.step(xv, y, frame_lengths=[20, 9], label_lengths=[3, 3])
    with pytest.raises(S2SArgumentError, match="22"):
        conv.step_ragged([x[0], x[1, :21]], [y[0], y[1]])
    with pytest.raises(S2SArgumentError):
        conv.step_ragged([x[0], x[1]], [y[0]])
    assert conv.decoder.frame_lengths is None and conv.encoder.rnn.lengths is None
    ys = [torch.tensor([1, 2, 10]), torch.tensor([3, 9])]
    with pytest.raises(ValueError, match="eos"):
        conv.Evaluate([x[0], x[1]], ys)
    with pytest.raises(ValueError, match="eos"):
        vgg.Evaluate([xv[0], xv[1]], [torch.tensor([1, 10]), torch.tensor([10])], eos=9)
    with pytest.raises(ValueError):
        conv.Evaluate([x[0], x[1]], ys[:1])
    with pytest.raises(S2SArgumentError):
        conv.BeamSearch(10)  # no annotations yet
