"""Beam search with hybrid location-aware attention on the shared-annotation path (Attention.share_hybrid_search,
s2s_attn_dims.beam_share_hybrid): the hypotheses of an utterance share its Vh and h, only ws and alpha_{t-1} stay
per hypothesis, and a padded batch is searched with frame lengths.

  bookkeeping   the scripted search of test_gpu_evaluate.py on a hybrid module: exact;
  arithmetic    the shared path against the replicated one on the same module and annotations;
  masking       a ragged batch against the per-utterance oracle, garbage on the padding frames;
  the model     ConvBiLSTMAttentionModel.Evaluate in one ragged search per batch against its equal-L' groups.
"""
import ctypes

import numpy as np
import pytest
import torch

import beam_script as bs
from oracle import frontend_oracle as fo
from oracle import s2s_oracle as orc
from paths import decisions

pytestmark = pytest.mark.gpu

TOL = 1e-4
S, A, SC, O, M, KWIN, NF = 32, 64, 64, 11, 4, 3, 8
EOS = 2


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


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


# --------------------------------------------------------------------------- the decoders under test

def _cfg(lstm, kW=5, outputDepth=O):
    return orc.ModelConfig(inputFrameSize=8, hiddenFrameSize=16, outputFrameSize=A // 2, scoreDepth=SC, stateDepth=S,
                           outputDepth=outputDepth, mlpDepth=M, maxoutWindow=KWIN, numLayers=1,
                           hybridAttendFilterSize=kW, hybridAttendFeatureMaps=NF, decoderLSTM=lstm)


def _params(cell, seed, kW=5, outputDepth=O):
    """(cfg, P) of a GRU or LSTM decoder with hybrid attention, fp32-representable: sharpened as the ragged tests of
    test_gpu_evaluate.py are, and hybU x 4 so the location features visibly steer the scores."""
    from test_gpu_evaluate import _sharpen
    if cell == "gru":
        cfg = _cfg(False, kW, outputDepth)
        P = orc.init_params(cfg, seed)
    else:
        from test_frontend import _lstm_dec_case
        cfg, P = _lstm_dec_case(np.random.default_rng(seed), S, A, SC, outputDepth, (kW, NF), "maxout")
    P["hybU"] = P["hybU"] * 4.0
    return cfg, _sharpen(P)


def _ext_layers(seed):
    rng = np.random.default_rng(1000 + seed)
    return [("linear", _f32(rng.standard_normal((2 * O, S + A)) * 0.6), _f32(rng.standard_normal(2 * O) * 0.1)),
            ("relu",),
            ("linear", _f32(rng.standard_normal((O, 2 * O)) * 0.9), _f32(rng.standard_normal(O) * 0.1)),
            ("logsoftmax",)]


def _load(s2s, fe, cell, P, cfg, layers=None):
    """The module for (cfg, P): fused MaxoutMLP, or the external Linear -> ReLU -> Linear -> LogSoftMax of `layers`
    (the stepwise entry points).  share_hybrid_search is left at its default."""
    Ov = cfg.outputDepth
    if layers is None:
        mlp = s2s.MaxoutMLP(S + A, M, KWIN, Ov)
    else:
        mlp = fe.Sequential(fe.Linear(S + A, 2 * Ov), fe.ReLU(), fe.Linear(2 * Ov, Ov), fe.LogSoftMax())
        with torch.no_grad():
            for m, lay in zip([m for m in mlp.modules if isinstance(m, fe.Linear)], (layers[0], layers[2])):
                m.weight.copy_(torch.tensor(lay[1]))
                m.bias.copy_(torch.tensor(lay[2]))
    if cell == "lstm":
        from test_frontend import _load_lstm_attention
        return _load_lstm_attention(s2s, fe, P, cfg, mlp)[0]
    att = s2s.Attention(s2s.GRU(S, S), mlp, SC, cfg.hybridAttendFilterSize, NF, S, A, Ov, True, 0.0)
    with torch.no_grad():
        for n in ("V", "Ws", "bs", "we", "Wy", "by", "Wc", "bc", "Wd", "bd", "hybW", "hybb", "hybU"):
            att.own[n].copy_(torch.tensor(P[n]).reshape(att.own[n].shape))
        for t, g in zip(att.decoder_recurrent.weight, "zrh"):
            t.copy_(torch.tensor(P["dec.W" + g]))
        if layers is None:
            for t, n in zip(mlp.weight, ("Wm", "bm", "Wo", "bo")):
                t.copy_(torch.tensor(P[n]).reshape(t.shape))
    return att.cuda()


# --------------------------------------------------------------------------- exact bookkeeping

RAGGED6 = [1, 15, 16, 17, 33, 40]


@pytest.mark.parametrize("K", [5, 1])
def test_scripted_ragged_search_is_exact_with_hybrid_attention(s2s, K):
    """test_gpu_evaluate.py::test_scripted_ragged_search_is_exact (B = 6, O = 9, L = 40, frame lengths and limits
    [1, 15, 16, 17, 33, 40]) on a hybrid Attention with share_hybrid_search: the log-probabilities are scripted, so
    tokens, lengths, -1 padding, scores (bitwise) and the finished lists must equal the reference search whatever
    the attention computes -- the per-hypothesis alpha buffers and their gather by parent sit in the same
    bookkeeping kernels."""
    from test_gpu_evaluate import ScriptedMLP
    Os, L, eos = 9, 40, 4
    table = bs.script_table(np.random.default_rng(200 + K), len(RAGGED6), K, Os, L, eos, eos_rates=(0.03, 0.12))
    B, maxlen = table.shape[1], table.shape[0] - 1
    torch.manual_seed(1)
    att = s2s.Attention(s2s.GRU(16, 16), ScriptedMLP(table), 16, 5, 8, 16, 16, Os, True, 0.0).cuda()
    att.share_hybrid_search = True
    h = cu(np.random.default_rng(5).standard_normal((B, L, 16)))
    with decisions() as dec:
        out = att.BeamSearch(h, eos, K, maxlen, finished=True, frame_lengths=RAGGED6, maxseqlengths=RAGGED6)
        torch.cuda.synchronize()
        assert dec["beam.attn.path"] == 1
    toks, lens, scores, nfin, flen, fscore, fseq = [t.cpu().numpy() for t in out]
    assert toks.shape == (B, maxlen + 1) and fseq.shape == (B, K, maxlen + 1)
    forced = []
    for b in range(B):
        fin, pred, score, trace = bs.reference_search(table[:, b], eos, K, RAGGED6[b])
        forced.append(any(r == "maxlen" for st in trace for _, _, r in st["finished"]))
        assert int(lens[b]) == len(pred) and toks[b, :lens[b]].tolist() == pred, (b, toks[b].tolist(), pred)
        assert (toks[b, lens[b]:] == -1).all(), (b, toks[b].tolist())
        assert _bits(scores[b]) == _bits(score), (b, float(scores[b]), score)
        assert int(nfin[b]) == len(fin), (b, int(nfin[b]), len(fin))
        for f, (seq, sc) in enumerate(fin):
            assert int(flen[b, f]) == len(seq) and fseq[b, f, :len(seq)].tolist() == seq, (b, f, seq)
            assert _bits(fscore[b, f]) == _bits(sc), (b, f, float(fscore[b, f]), sc)
    assert forced[0] and sum(forced) >= 2  # hypotheses reach their utterance's own limit


# --------------------------------------------------------------------------- shared equals replicated, no lengths

LONG_L = 160
# (cell, kW, K, outputDepth, L, parameter seed).  kW = 4: the even filter pads asymmetrically (hyb_pad_left);
# K = 16 / O = 17: all sixteen accumulators of the score loop; L = 160: ten chunks, the overlaid layout.  Seeds chosen
# on the CPU with the oracle: at least two utterances of each case never prefer eos and run to the length limit.
AB_CASES = [("gru", 5, 5, O, 40, 4), ("lstm", 5, 5, O, 40, 3), ("gru", 4, 5, O, 40, 5), ("lstm", 4, 5, O, 40, 1),
            ("gru", 5, 16, 17, 40, 4), ("gru", 5, 5, O, LONG_L, 4)]


def _ab_case(cell, kW, Ov, L, seed):
    cfg, P = _params(cell, seed, kW, Ov)
    h = _f32(np.random.default_rng(seed).standard_normal((4, L, A)) * 1.5)
    return cfg, P, h


@pytest.mark.parametrize("cell,kW,K,Ov,L,seed", AB_CASES)
def test_shared_path_equals_replicated_path(s2s, fe, cell, kW, K, Ov, L, seed):
    """The same module and annotations (B = 4, no lengths) with share_hybrid_search on and off: the two attention
    kernels form every (row, frame) score in the same operation order, so tokens and lengths are identical and the
    scores agree to 1e-6 relative (the bound of test_overlaid_layout_equals_replicated_path; what may differ is the
    Vh GEMM's shape, (B L) rows against (B K L))."""
    cfg, P, h = _ab_case(cell, kW, Ov, L, seed)
    att = _load(s2s, fe, cell, P, cfg)
    hd = cu(h)
    runs = {}
    for on in (True, False):
        att.share_hybrid_search = on
        with decisions() as dec:
            runs[on] = [t.cpu() for t in att.BeamSearch(hd, EOS, K, L)]
            torch.cuda.synchronize()
            assert dec["beam.attn.path"] == (1 if on else 0)
            assert dec["beam.layout.overlay"] == (1 if on and L == LONG_L else 0)
    shared, repl = runs[True], runs[False]
    a, b = shared[2].double().numpy(), repl[2].double().numpy()
    print(f"{cell} kW = {kW} K = {K} L = {L}: lengths {shared[1].tolist()}, scores bitwise equal = "
          f"{bool(torch.equal(shared[2], repl[2]))}, max rel diff {np.abs(a - b).max() / np.abs(b).max():.3e}")
    assert torch.equal(shared[0], repl[0]) and torch.equal(shared[1], repl[1])
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
    if L == LONG_L:
        assert int(shared[1].max()) > 16  # the overlaid buffers are refilled again and again


# --------------------------------------------------------------------------- ragged against the oracle

LENS7 = [1, 3, 15, 16, 17, 33, 40]  # shorter than the filter, both sides of the 16-frame chunk edge, full length
# seeds chosen on the CPU: every assertion of _ragged_case holds
RAGGED_SEED = {"gru": 4, "lstm-ext": 3}
_cache = {}


def _ragged_case(kind, seed=None):
    """(cell, cfg, P, layers, ext, h, refs), computed once.  Before anything runs on the GPU: the fp32 and fp64
    oracle searches agree on every prediction (no near tie of the case's own), the case can see a missing mask
    (_oracle_ragged's leak check) and it can see missing location features (rescoring with hybU = 0 moves every
    multi-frame utterance's score by more than 100x the tolerance)."""
    from test_gpu_evaluate import _oracle_ragged, _ragged_h, _rescore
    key = (kind, seed)
    if key in _cache:
        return _cache[key]
    sd = RAGGED_SEED[kind] if seed is None else seed
    cell = "gru" if kind == "gru" else "lstm"
    cfg, P = _params(cell, sd)
    layers = _ext_layers(sd) if kind == "lstm-ext" else None
    ext = None if layers is None else (lambda v: fo.mlp_fwd(v[None], layers)[0][0])
    h = _ragged_h(np.random.default_rng(sd), len(LENS7), 40, A, LENS7)
    refs = _oracle_ragged(h, LENS7, P, cfg, EOS, 5, mlp=ext)
    assert sum(len(seq) > 1 for seq, _ in refs) >= 4, "most predictions must pass through the location features"
    P32 = {n: v.astype(np.float32) for n, v in P.items()}
    ext32 = None
    if layers is not None:
        l32 = [tuple(a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in lay) for lay in layers]
        ext32 = lambda v: fo.mlp_fwd(v[None], l32)[0][0]  # noqa: E731
    P0 = dict(P, hybU=np.zeros_like(P["hybU"]))
    for b, Lb in enumerate(LENS7):
        seq32, _ = orc.beam_search(h[b, :Lb].astype(np.float32), P32, cfg, EOS, 5, maxseqlength=Lb, mlp=ext32)
        assert [int(t) for t in seq32] == refs[b][0], f"fp32 and fp64 oracle predictions differ ({b}): another seed"
        if Lb > 1 and len(refs[b][0]) > 1:
            gap = abs(_rescore(h[b, :Lb], refs[b][0], P0, cfg, ext) - refs[b][1])
            assert gap > 100 * TOL * max(1.0, abs(refs[b][1])), (b, Lb, gap)
    _cache[key] = (cell, cfg, P, layers, ext, h, refs)
    return _cache[key]


@pytest.mark.parametrize("kind", ["gru", "lstm-ext"])
def test_ragged_hybrid_search_matches_the_oracle(s2s, fe, kind):
    """B = 7, L = 40, lengths [1, 3, 15, 16, 17, 33, 40], K = 5, finite garbage at 3x scale on the padding frames,
    judged by test_gpu_evaluate.py::_check_ragged (TOL = 1e-4): the reported score is the oracle's rescoring of the
    device's own prediction on the utterance's own frames, at most one prediction differs from the oracle's, and
    that one ties the oracle's best.  The GRU decoder with the fused MLP (s2s_attn_beam_search_ragged) and the LSTM
    decoder with an external MLP (the stepwise entry points).  Zeros in place of the garbage change no bit."""
    from test_gpu_evaluate import _check_ragged
    cell, cfg, P, layers, ext, h, refs = _ragged_case(kind)
    att = _load(s2s, fe, cell, P, cfg, layers)
    att.share_hybrid_search = True
    _check_ragged(att, h, LENS7, P, cfg, EOS, 5, refs, mlp=ext, overlay=0)
    hz = h.copy()
    for b, Lb in enumerate(LENS7):
        hz[b, Lb:] = 0.0
    garb = att.BeamSearch(cu(h), EOS, 5, 40, frame_lengths=LENS7)
    zero = att.BeamSearch(cu(hz), EOS, 5, 40, frame_lengths=LENS7)
    assert all(torch.equal(g, z) for g, z in zip(garb, zero))


# --------------------------------------------------------------------------- opt-in only

def test_frame_lengths_stay_refused_without_the_attribute(s2s):
    att = s2s.Attention(s2s.GRU(S, S), s2s.MaxoutMLP(S + A, M, KWIN, O), SC, 5, NF, S, A, O, True, 0.0).cuda()
    assert att.share_hybrid_search is False
    h = cu(np.random.default_rng(0).standard_normal((2, 20, A)))
    with pytest.raises(ValueError, match="hybrid"):
        att.BeamSearch(h, EOS, 3, 8, frame_lengths=[20, 10])
    from s2s_amd import _lib
    d = att._dims(h, 1)
    assert d.beam_share_hybrid == 0
    fl = cu([20, 10], torch.int32)
    d.frame_lengths = fl.data_ptr()
    ws = torch.empty(_lib.lib.s2s_attn_beam_workspace_bytes(ctypes.byref(d), 3, 8), dtype=torch.uint8, device="cuda")
    rc = _lib.lib.s2s_attn_beam_init(s2s.nn.get_context(0).handle, s2s.nn.stream_ptr(), ctypes.byref(d),
                                     ctypes.c_void_p(h.data_ptr()), att._ptrs(False), EOS, 3, 8,
                                     ctypes.c_void_p(ws.data_ptr()), ws.numel())
    err = _lib.lib.s2s_last_error()
    assert rc != 0 and b"hybrid" in err and b"beam_share_hybrid" in err


# --------------------------------------------------------------------------- the model

def test_conv_model_evaluates_in_one_ragged_search_per_batch(s2s, fe):
    """test_gpu_models_ragged.py's conv + BiLSTM Evaluate case (7 utterances, batches of at most 4) with
    decoder.share_hybrid_search: one search per padded batch, and against the equal-L' groups of the same model the
    same numCorrect and distances, nll bitwise, predictions identical (or at most one differing, which must tie the
    oracle's best under the near-tie rule).  Garbage on the padding frames of x changes no bit."""
    from s2s_amd.data import PackedUtterances
    from test_gpu_models_ragged import RTOL, _eval_case, _rescore
    model, c, xs, ys, eos, ref, Pb, ext, factor = _eval_case(s2s, fe, "conv")
    cfg = c["cfg"]
    xd, yd = [cu(x) for x in xs], [torch.tensor(y) for y in ys]

    class GarbagePadding(PackedUtterances):
        def batch(self, idx, Lmax=None, Tmax=None, out=None):
            bt = super().batch(idx, Lmax, Tmax, out)
            g = torch.Generator(device="cuda").manual_seed(1)
            for j, L in enumerate(bt[4]):
                pad = bt[0][j, L:]
                pad.copy_(torch.randn(pad.shape, generator=g, device="cuda") * 30)
            return bt

    assert model.decoder.share_hybrid_search is False
    acc_g, nll_g, per_g, preds_g = model.Evaluate(xd, yd, K=5, max_batch=4)
    det_g, groups_g = dict(model.eval_detail), list(model.eval_groups)
    assert groups_g == [(1, [0]), (3, [1, 2, 3]), (4, [0]), (5, [1, 2])], groups_g
    model.decoder.share_hybrid_search = True
    try:
        with decisions() as dec:
            acc, nll, per, preds = model.Evaluate(xd, yd, K=5, max_batch=4)
            assert dec["beam.attn.path"] == 1
        det = dict(model.eval_detail)
        assert model.eval_groups == [(None, [0, 1, 2, 3]), (None, [0, 1, 2])], model.eval_groups
        first = (acc, nll, per, [p.tolist() for p in preds], det)
        acc2, nll2, per2, preds2 = model.Evaluate(GarbagePadding(xs, ys), None, K=5, max_batch=4)
        assert (acc2, nll2, per2, [p.tolist() for p in preds2], model.eval_detail) == first
    finally:
        model.decoder.share_hybrid_search = False
    assert det["numCorrect"] == det_g["numCorrect"] and det["dist"] == det_g["dist"]
    assert (_bits(det["nll"]) == _bits(det_g["nll"])).all() and acc == acc_g and nll == nll_g and per == per_g
    differ = [i for i in range(len(xs)) if preds[i].tolist() != preds_g[i].tolist()]
    sg, sr = np.array(det_g["score"]), np.array(det["score"])
    print(f"ragged vs grouped: {len(differ)} predictions differ, max rel score diff "
          f"{(np.abs(sr - sg) / np.maximum(1.0, np.abs(sg))).max():.3e}")
    assert len(differ) <= 1
    for i, r in enumerate(ref):
        seq = preds[i].tolist()
        mine = _rescore(r["h"], seq, Pb, cfg, ext)
        assert abs(mine - det["score"][i]) <= RTOL * max(1.0, abs(mine)), (i, mine, det["score"][i])
        if i in differ:
            assert abs(mine - r["score"]) <= RTOL * max(1.0, abs(r["score"])), (i, seq, r["seq"], mine, r["score"])
