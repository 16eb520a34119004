"""Validation on the device (timit/timit.lua:368-417): the ragged-batch beam search on the shared-annotation
attention kernel (beam_f2_shared), the forward-only model step, and ChorowskiBaseline.Evaluate.

Scripted searches (tests/beam_script.py) are compared exactly; searches the real decoder steers are judged by the
near-tie rule of tests/test_frontend.py::_check_beam, here in both directions: at least B - 1 predictions
identical, a differing one within 1e-4 relative of the oracle's best, the reported score within 1e-4 relative
of the oracle's rescoring of the device's own prediction."""
import ctypes
import os

import numpy as np
import pytest
import torch

import beam_script as bs
from oracle import s2s_oracle as orc
from paths import decisions

pytestmark = pytest.mark.gpu
TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    return t.double().cpu().numpy()


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


# --------------------------------------------------------------------------- scripted ragged search, exact

class ScriptedMLP:
    """decoder_mlp returning the next count's (B*K, O) rows of a (maxlen + 1, B, K, O) table (test_gpu_decode.py)."""

    def __init__(self, table):
        n, B, K, O = table.shape
        self.table = cu(table.reshape(n, B * K, O))
        self.rows = []

    def forward(self, rows):
        self.rows.append(rows.clone())
        return self.table[len(self.rows) - 1]

    def backward(self, input, gradOutput, scale=1.0):
        raise AssertionError("the search never runs the decoder_mlp backward")

    def parameters(self):
        return [], []


def _scripted(s2s, table, eos, K, L, frame_lengths, maxlens):
    """Runs the scripted search on (B, L, 16) annotations and compares every utterance with the reference search
    under its own limit: tokens, length, -1 padding, score (bitwise) and the whole finished list."""
    B, O = table.shape[1], table.shape[3]
    maxlen = table.shape[0] - 1
    torch.manual_seed(1)
    mlp = ScriptedMLP(table)
    att = s2s.Attention(s2s.GRU(16, 16), mlp, 16, 0, 0, 16, 16, O, True, 0.0).cuda()
    h = cu(np.random.default_rng(5).standard_normal((B, L, 16)))
    with decisions() as dec:
        out = att.BeamSearch(h, eos, K, maxlen, finished=True, frame_lengths=frame_lengths, maxseqlengths=maxlens)
        torch.cuda.synchronize()
        assert dec["beam.attn.path"] == 1
    toks, lens, scores, nfin, flen, fscore, fseq = [t.cpu().numpy() for t in out]
    assert toks.shape == (B, maxlen + 1) and fseq.shape == (B, K, maxlen + 1)
    traces = []
    for b in range(B):
        fin, pred, score, trace = bs.reference_search(table[:, b], eos, K, int(maxlens[b]))
        traces.append(trace)
        assert int(lens[b]) == len(pred) and toks[b, :lens[b]].tolist() == pred, (b, toks[b].tolist(), pred)
        assert (toks[b, lens[b]:] == -1).all(), (b, toks[b].tolist())
        assert _bits(scores[b]) == _bits(score), (b, float(scores[b]), score)
        assert int(nfin[b]) == len(fin), (b, int(nfin[b]), len(fin))
        for f, (seq, sc) in enumerate(fin):
            assert int(flen[b, f]) == len(seq) and fseq[b, f, :len(seq)].tolist() == seq, (b, f, seq)
            assert _bits(fscore[b, f]) == _bits(sc), (b, f, float(fscore[b, f]), sc)
    return traces, mlp


RAGGED6 = [1, 15, 16, 17, 33, 40]


@pytest.mark.parametrize("K", [5, 1])
def test_scripted_ragged_search_is_exact(s2s, K):
    """B = 6, O = 9, L = 40, frame lengths and limits [1, 15, 16, 17, 33, 40]: every utterance equals the
    reference search under its own limit.  The eos rates are low enough that hypotheses reach their utterance's
    limit (asserted from the reference's trace), which only the per-utterance maxlen explains."""
    O, L, eos = 9, 40, 4
    table = bs.script_table(np.random.default_rng(200 + K), len(RAGGED6), K, O, L, eos, eos_rates=(0.03, 0.12))
    traces, _ = _scripted(s2s, table, eos, K, L, RAGGED6, RAGGED6)
    forced = [any(r == "maxlen" for st in tr for _, _, r in st["finished"]) for tr in traces]
    assert forced[0] and sum(forced) >= 2
    assert len({tr[-1]["count"] for tr in traces}) >= 3  # the utterances end at different counts


def test_limit_one_among_long_utterances(s2s):
    """One utterance's limit is 1 while the others never see eos and run to 40: it is done at count 1, between the
    host's polls at counts 3, 7, ..., and the 39 further steps leave its K finished hypotheses untouched."""
    K, O, L, eos = 3, 9, 40, 2
    table = bs.script_table(np.random.default_rng(210), 4, K, O, L, eos)
    table[..., eos] = -np.inf
    limits = [40, 1, 40, 40]
    traces, mlp = _scripted(s2s, table, eos, K, L, None, limits)
    assert traces[1][-1]["count"] == 1 and len(traces[1][-1]["finished"]) + len(traces[1][0]["finished"]) == K
    assert len(mlp.rows) == L + 1  # the host stepped on to the last count


# --------------------------------------------------------------------------- the real decoder, ragged

def _decoder_cfg(S, A, Sc, O, M, Kw, lstm=False):
    return orc.ModelConfig(inputFrameSize=8, hiddenFrameSize=16, outputFrameSize=A // 2, scoreDepth=Sc, stateDepth=S,
                           outputDepth=O, mlpDepth=M, maxoutWindow=Kw, numLayers=1, decoderLSTM=lstm)


def _sharpen(P):
    """Wo, Wy, Wm, we x 3: log-probabilities far from uniform, attention far from flat, so padding frames that
    leak into the context move the scores visibly."""
    for n in ("Wo", "Wy", "Wm", "we"):
        if n in P:
            P[n] = P[n] * 3.0
    return {n: _f32(v) for n, v in P.items()}


def _ragged_h(rng, B, L, A, lens):
    """Real frames at scale 1.5; padding frames hold finite garbage at 3x that scale."""
    h = rng.standard_normal((B, L, A)) * 1.5
    for b, Lb in enumerate(lens):
        h[b, Lb:] = rng.standard_normal((L - Lb, A)) * 4.5
    return _f32(h)


def _rescore(hb, seq, P, cfg, mlp=None):
    st, Vh, tot, y = orc.decoder_zero_state(hb.shape[0], cfg.stateDepth), hb @ P["V"].T, 0.0, -1
    for tok in seq:
        lp, st = orc.decoder_step(hb, Vh, st, y, P, cfg, mlp)
        tot, y = tot + lp[tok], tok
    return tot


def _oracle_ragged(h, lens, P, cfg, eos, K, mlp=None):
    """Per utterance, on its own frames with its own limit; and -- before anything runs on the GPU -- the proof
    that this case can see a missing mask: rescoring the oracle's prediction on the padded annotations differs
    from rescoring on the utterance's own frames by more than 100x the score tolerance."""
    refs = []
    for b, Lb in enumerate(lens):
        seq, score = orc.beam_search(h[b, :Lb], P, cfg, eos, K, maxseqlength=Lb, mlp=mlp)
        if Lb < h.shape[1]:
            leak = abs(_rescore(h[b], seq, P, cfg, mlp) - _rescore(h[b, :Lb], seq, P, cfg, mlp))
            assert leak > 100 * TOL * max(1.0, abs(score)), (b, Lb, leak, score)
        refs.append((list(seq), score))
    return refs


def _check_ragged(att, h, lens, P, cfg, eos, K, refs, mlp=None, overlay=None):
    B, L = h.shape[0], h.shape[1]
    with decisions() as dec:
        toks, ln, sc = att.BeamSearch(cu(h), eos, K, L, frame_lengths=lens)
        torch.cuda.synchronize()
        assert dec["beam.attn.path"] == 1
        assert overlay is None or dec["beam.layout.overlay"] == overlay
    toks, ln, sc = toks.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()
    agree = 0
    for b, Lb in enumerate(lens):
        seq = [int(t) for t in toks[b, :ln[b]]]
        assert all(t == -1 for t in toks[b, ln[b]:])
        assert seq[-1] == eos or len(seq) == Lb + 1, (b, seq)
        ref_seq, ref_score = refs[b]
        mine = _rescore(h[b, :Lb], seq, P, cfg, mlp)
        print(f"utterance {b} (L_b = {Lb}): score {sc[b]:.6f}, oracle rescoring {mine:.6f}, oracle best "
              f"{ref_score:.6f}, {'same' if seq == ref_seq else 'different'} prediction")
        assert abs(mine - sc[b]) <= TOL * max(1.0, abs(mine)), (b, mine, sc[b])
        if seq == ref_seq:
            agree += 1
        else:
            assert abs(mine - ref_score) <= TOL * max(1.0, abs(ref_score)), (b, seq, ref_seq, mine, ref_score)
    assert agree >= B - 1


def _load_gru_attention(s2s, P, cfg, mlp):
    S, A, Sc, O = cfg.stateDepth, cfg.annotationDepth, cfg.scoreDepth, cfg.outputDepth
    att = s2s.Attention(s2s.GRU(S, S), mlp, Sc, 0, 0, S, A, O, True, 0.0)
    with torch.no_grad():
        for n in ("V", "Ws", "bs", "we", "Wy", "by", "Wc", "bc", "Wd", "bd"):
            att.own[n].copy_(torch.tensor(P[n]).reshape(att.own[n].shape))
        for t, g in zip(att.decoder_recurrent.weight, "zrh"):
            t.copy_(torch.tensor(P["dec.W" + g]))
        if isinstance(mlp, s2s.MaxoutMLP):
            for t, n in zip(mlp.weight, ("Wm", "bm", "Wo", "bo")):
                t.copy_(torch.tensor(P[n]).reshape(t.shape))
    return att.cuda()


SMALL = dict(S=32, A=64, Sc=64, O=11, M=4, Kw=3)
LENS7 = [1, 5, 15, 16, 17, 33, 40]
# seeds chosen on the CPU: the mask-visibility property above holds for every padded utterance, and the float32 and
# float64 oracle searches agree on every prediction (no near tie to begin with)
SEED_SMALL = {1: 3, 5: 3}
SEED_WIDE, SEED_LSTM, SEED_EXT = 2, 3, 3
_cache = {}


def _small_case(K):
    """Shared by the tests that need it; computed once."""
    key = ("small", K)
    if key not in _cache:
        cfg = _decoder_cfg(**SMALL)
        P = _sharpen(orc.init_params(cfg, SEED_SMALL[K]))
        h = _ragged_h(np.random.default_rng(SEED_SMALL[K]), len(LENS7), 40, SMALL["A"], LENS7)
        _cache[key] = (cfg, P, h, _oracle_ragged(h, LENS7, P, cfg, 2, K))
    return _cache[key]


@pytest.mark.parametrize("K", [1, 5])
def test_ragged_search_small_widths(s2s, K):
    """A = Sc = 64, S = 32, O = 11, B = 7, L = 40, lengths [1, 5, 15, 16, 17, 33, 40]: a length of 1, the chunk
    edge at 15 / 16 / 17, and two chunks wholly past L_b."""
    cfg, P, h, refs = _small_case(K)
    att = _load_gru_attention(s2s, P, cfg, s2s.MaxoutMLP(SMALL["S"] + SMALL["A"], SMALL["M"], SMALL["Kw"], SMALL["O"]))
    _check_ragged(att, h, LENS7, P, cfg, 2, K, refs)


def test_ragged_search_reference_widths(s2s):
    """A = Sc = 512, S = 256, O = 62, M = 64, window 7, B = 4, L = 48, lengths [7, 16, 31, 48], K = 5: two float4
    of a Vh row per lane."""
    cfg = _decoder_cfg(256, 512, 512, 62, 64, 7)
    lens, eos = [7, 16, 31, 48], 23
    P = _sharpen(orc.init_params(cfg, SEED_WIDE))
    h = _ragged_h(np.random.default_rng(SEED_WIDE), 4, 48, 512, lens)
    refs = _oracle_ragged(h, lens, P, cfg, eos, 5)
    att = _load_gru_attention(s2s, P, cfg, s2s.MaxoutMLP(256 + 512, 64, 7, 62))
    _check_ragged(att, h, lens, P, cfg, eos, 5, refs)


def test_ragged_search_lstm_decoder(s2s, fe):
    from test_frontend import _load_lstm_attention, _lstm_dec_case
    S, A, Sc, O = SMALL["S"], SMALL["A"], SMALL["Sc"], SMALL["O"]
    rng = np.random.default_rng(SEED_LSTM)
    cfg, P = _lstm_dec_case(rng, S, A, Sc, O, (0, 0), "maxout")
    P = _sharpen(P)
    h = _ragged_h(rng, len(LENS7), 40, A, LENS7)
    refs = _oracle_ragged(h, LENS7, P, cfg, 2, 5)
    att, _ = _load_lstm_attention(s2s, fe, P, cfg, s2s.MaxoutMLP(S + A, 4, 3, O))
    _check_ragged(att, h, LENS7, P, cfg, 2, 5, refs)


def test_ragged_search_external_mlp(s2s, fe):
    """The external decoder_mlp Linear -> ReLU -> Linear -> LogSoftMax between the search's step and advance calls
    (s2s_attn_beam_set_maxlens on the stepwise path)."""
    from oracle import frontend_oracle as fo
    S, A, Sc, O = SMALL["S"], SMALL["A"], SMALL["Sc"], SMALL["O"]
    cfg = _decoder_cfg(**SMALL)
    rng = np.random.default_rng(SEED_EXT)
    P = _sharpen(orc.init_params(cfg, SEED_EXT))
    layers = [("linear", _f32(rng.standard_normal((2 * O, S + A)) * 0.6), _f32(rng.standard_normal(2 * O) * 0.1)),
              ("relu",),
              ("linear", _f32(rng.standard_normal((O, 2 * O)) * 0.9), _f32(rng.standard_normal(O) * 0.1)),
              ("logsoftmax",)]
    ext = lambda v: fo.mlp_fwd(v[None], layers)[0][0]  # noqa: E731
    h = _ragged_h(rng, len(LENS7), 40, A, LENS7)
    refs = _oracle_ragged(h, LENS7, P, cfg, 2, 5, mlp=ext)
    mlp = fe.Sequential(fe.Linear(S + A, 2 * O), fe.ReLU(), fe.Linear(2 * O, O), fe.LogSoftMax())
    lins = [m for m in mlp.modules if isinstance(m, fe.Linear)]
    with torch.no_grad():
        for m, lay in zip(lins, (layers[0], layers[2])):
            m.weight.copy_(torch.tensor(lay[1]))
            m.bias.copy_(torch.tensor(lay[2]))
    att = _load_gru_attention(s2s, P, cfg, mlp)
    _check_ragged(att, h, LENS7, P, cfg, 2, 5, refs, mlp=ext)


# L = 160 at the small widths: 10 chunks, so the chunk partials PC (R x 10 x 64 floats) hold the buffers a step
# writes after the chunk combine (RHX, CY, gates, Maxout, log-probabilities, U: 510 floats per row and their
# alignment) -- the layout every utterance of realistic length gets, and the one tests/test_evaluate_cpu.py sizes
LONG_L, LENS_LONG = 160, [1, 17, 64, 95, 129, 144, 160]
SEED_LONG = 3


def _long_case(K):
    key = ("long", K)
    if key not in _cache:
        cfg = _decoder_cfg(**SMALL)
        P = _sharpen(orc.init_params(cfg, SEED_LONG))
        h = _ragged_h(np.random.default_rng(SEED_LONG), len(LENS_LONG), LONG_L, SMALL["A"], LENS_LONG)
        _cache[key] = (cfg, P, h, _oracle_ragged(h, LENS_LONG, P, cfg, 2, K))
    return _cache[key]


@pytest.mark.parametrize("K", [1, 5])
def test_ragged_search_with_the_overlaid_layout(s2s, K):
    """The ragged search against the per-utterance oracle where the step's post-combine buffers live inside the
    chunk partials, which every step's attention launch overwrites: a write moved in front of dec_f3_combine, or a
    read moved behind the next beam_f2_shared, shows here.  beam.layout.overlay proves the layout ran; at L = 40
    (the tests above) it must not."""
    cfg, P, h, refs = _long_case(K)
    mk = lambda: _load_gru_attention(  # noqa: E731
        s2s, P, cfg, s2s.MaxoutMLP(SMALL["S"] + SMALL["A"], SMALL["M"], SMALL["Kw"], SMALL["O"]))
    _check_ragged(mk(), h, LENS_LONG, P, cfg, 2, K, refs, overlay=1)
    cfg, P, h, refs = _small_case(K)
    _check_ragged(mk(), h, LENS7, P, cfg, 2, K, refs, overlay=0)


def test_overlaid_layout_equals_replicated_path(s2s):
    """Equal lengths at L = 160, B = 6, K = 5: the shared path on the overlaid layout against the replicated path
    (its own buffers, no overlay): tokens and lengths identical, scores to 1e-6 relative."""
    from s2s_amd._lib import lib
    lib.s2s_debug_beam_replicate.argtypes, lib.s2s_debug_beam_replicate.restype = [ctypes.c_int], None
    cfg = _decoder_cfg(**SMALL)
    P = _sharpen(orc.init_params(cfg, 9))
    h = cu(_f32(np.random.default_rng(9).standard_normal((6, LONG_L, SMALL["A"])) * 1.5))
    att = _load_gru_attention(s2s, P, cfg, s2s.MaxoutMLP(SMALL["S"] + SMALL["A"], SMALL["M"], SMALL["Kw"], SMALL["O"]))
    with decisions() as dec:
        shared = [t.cpu() for t in att.BeamSearch(h, 2, 5, LONG_L)]
        assert dec["beam.attn.path"] == 1 and dec["beam.layout.overlay"] == 1
    lib.s2s_debug_beam_replicate(1)
    try:
        with decisions() as dec:
            repl = [t.cpu() for t in att.BeamSearch(h, 2, 5, LONG_L)]
            assert dec["beam.attn.path"] == 0 and dec["beam.layout.overlay"] == 0
    finally:
        lib.s2s_debug_beam_replicate(0)
    assert torch.equal(shared[0], repl[0]) and torch.equal(shared[1], repl[1])
    assert int(shared[1].max()) > 16  # searches of many steps: the buffers are refilled again and again
    a, b = shared[2].double().numpy(), repl[2].double().numpy()
    print(f"overlaid vs replicated scores: bitwise equal = {bool(torch.equal(shared[2], repl[2]))}, "
          f"max rel diff {np.abs(a - b).max() / np.abs(b).max():.3e}")
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()


def test_frame_lengths_with_hybrid_attention_are_refused(s2s):
    att = s2s.Attention(s2s.GRU(32, 32), s2s.MaxoutMLP(96, 4, 3, 11), 64, 5, 8, 32, 64, 11, True, 0.0).cuda()
    h = cu(np.random.default_rng(0).standard_normal((2, 20, 64)))
    with pytest.raises(ValueError, match="hybrid"):
        att.BeamSearch(h, 2, 3, 8, frame_lengths=[20, 10])
    # the C entry itself says so
    from s2s_amd import _lib
    d = att._dims(h, 1)
    fl = cu([20, 10], torch.int32)
    d.frame_lengths = fl.data_ptr()
    ws = torch.empty(_lib.lib.s2s_attn_beam_workspace_bytes(ctypes.byref(d), 3, 8), dtype=torch.uint8, device="cuda")
    rc = _lib.lib.s2s_attn_beam_init(s2s.nn.get_context(0).handle, s2s.nn.stream_ptr(), ctypes.byref(d),
                                     ctypes.c_void_p(h.data_ptr()), att._ptrs(False), 2, 3, 8,
                                     ctypes.c_void_p(ws.data_ptr()), ws.numel())
    assert rc != 0 and b"hybrid" in _lib.lib.s2s_last_error()


def test_training_frame_lengths_are_not_picked_up(s2s):
    """att.frame_lengths (the training attribute) never reaches the search: the result equals a module's without."""
    cfg, P, h, _ = _small_case(5)
    mk = lambda: _load_gru_attention(  # noqa: E731
        s2s, P, cfg, s2s.MaxoutMLP(SMALL["S"] + SMALL["A"], SMALL["M"], SMALL["Kw"], SMALL["O"]))
    a, b = mk(), mk()
    b.frame_lengths = LENS7
    for x, y in zip(a.BeamSearch(cu(h), 2, 5, 12), b.BeamSearch(cu(h), 2, 5, 12)):
        assert torch.equal(x, y)
    assert b.frame_lengths == LENS7


# --------------------------------------------------------------------------- equal lengths are unchanged

def _equal_case(s2s):
    cfg = _decoder_cfg(**SMALL)
    P = _sharpen(orc.init_params(cfg, 7))
    h = _f32(np.random.default_rng(7).standard_normal((6, 30, SMALL["A"])) * 1.5)
    att = _load_gru_attention(s2s, P, cfg, s2s.MaxoutMLP(SMALL["S"] + SMALL["A"], SMALL["M"], SMALL["Kw"], SMALL["O"]))
    return att, cu(h)


def test_full_frame_lengths_equal_no_lengths(s2s):
    att, h = _equal_case(s2s)
    plain = att.BeamSearch(h, 2, 5, 30)
    full = att.BeamSearch(h, 2, 5, 30, frame_lengths=[30] * 6)
    for a, b in zip(plain, full):
        assert torch.equal(a, b)  # tokens, lengths, and the scores bit for bit


def test_shared_path_equals_replicated_path(s2s):
    """B = 6, L = 30, K = 5: the shared kernel against the replicated path (debug knob): tokens and lengths
    identical, scores to 1e-6 relative; beam.attn.path proves which arm ran."""
    from s2s_amd._lib import lib
    lib.s2s_debug_beam_replicate.argtypes, lib.s2s_debug_beam_replicate.restype = [ctypes.c_int], None
    att, h = _equal_case(s2s)
    with decisions() as dec:
        shared = [t.cpu() for t in att.BeamSearch(h, 2, 5, 30)]
        assert dec["beam.attn.path"] == 1
    lib.s2s_debug_beam_replicate(1)
    try:
        with decisions() as dec:
            repl = [t.cpu() for t in att.BeamSearch(h, 2, 5, 30)]
            assert dec["beam.attn.path"] == 0
    finally:
        lib.s2s_debug_beam_replicate(0)
    assert torch.equal(shared[0], repl[0]) and torch.equal(shared[1], repl[1])
    a, b = shared[2].double().numpy(), repl[2].double().numpy()
    print(f"shared vs replicated scores: bitwise equal = {bool(torch.equal(shared[2], repl[2]))}, "
          f"max rel diff {np.abs(a - b).max() / np.abs(b).max():.3e}")
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()


# --------------------------------------------------------------------------- forward-only model step

def _golden_inputs():
    """The tiny golden case's inputs (B = 4, L = 10, T = 9, F = 5, O = 7, Maxout 3 x 2, 3 layers).  Its hidden, state
    and score widths (4, 4, 5) are below what the library runs (multiples of 16 -- s2s_model_workspace_bytes
    refuses them), so those are raised to 16, the smallest it accepts, with the model's own initialisation."""
    g = np.load(os.path.join(GOLDEN, "tiny_step.npz"))
    kw = {k: (float(g["cfg_" + k]) if k == "penalty" else int(g["cfg_" + k]))
          for k in ("inputFrameSize", "outputDepth", "mlpDepth", "maxoutWindow", "penalty", "numLayers")}
    kw.update(hiddenFrameSize=16, outputFrameSize=16, scoreDepth=16, stateDepth=16)
    return kw, g["x"], g["labels"], None


def _fwd_case(s2s, case):
    if case == "golden_inputs_w16":
        kw, x, labels, params = _golden_inputs()
        return s2s.ModelConfig(**kw), x, labels, params
    cfg = orc.ModelConfig()  # config 2's widths
    x, labels = orc.synthetic_batch(cfg, 4, 32, 10, seed=77, pad=4, eos=23, dtype=np.float32)
    return s2s.ModelConfig(), x, labels, None


MODES = {"eager": dict(), "overlap": dict(overlap=True), "graph": dict(graph=True, overlap=True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("lengths", [False, True])
@pytest.mark.parametrize("case", ["config2", "golden_inputs_w16"])
def test_forward_only_equals_the_step(s2s, case, lengths, mode):
    """logp, nll and encoder_output() of forward() are bitwise those of a full step() on the same inputs, with and
    without lengths, eagerly (one stream / side-stream layout) and as a captured and replayed graph; a
    sentinel-filled gradient buffer is untouched (the library is handed NULL)."""
    cfg, x, labels, params = _fwd_case(s2s, case)
    m = s2s.ChorowskiBaseline(cfg, seed=5, **MODES[mode])
    if params is not None:
        m.params.copy_(torch.tensor(params, dtype=torch.float32))
    xd, ld = cu(x), cu(labels, torch.int32)
    B, L, T = xd.shape[0], xd.shape[1], ld.shape[1]
    kw = {}
    if lengths:
        kw = dict(frame_lengths=[max(1, L - 3 * b) for b in range(B)], label_lengths=[max(1, T - b) for b in range(B)])
    # on a stream of its own: a graph-mode context captures and replays only on a non-default stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(2):  # (graph mode: a capture, then a replay)
            nll_s, logp_s = m.step(xd, ld, normalizeNLL=False, stream=st, **kw)
        nll_s, logp_s = nll_s.clone(), logp_s.clone()
        enc_s, alpha_s = m.encoder_output().clone(), m.decoder_alpha().clone()
        m.grads.fill_(7.25)
        for _ in range(2):
            nll_f, logp_f = m.forward(xd, ld, stream=st, **kw)
        st.synchronize()
        assert torch.equal(logp_f, logp_s) and torch.equal(nll_f, nll_s)
        assert torch.equal(m.encoder_output(), enc_s) and torch.equal(m.decoder_alpha(), alpha_s)
        assert bool((m.grads == 7.25).all())
        if mode == "graph":  # two keys (the flag is part of it), each captured once and replayed twice
            captures, replays, cached = m.ctx.graph_stats()
            assert (captures, replays, cached) == (2, 4, 2)
        nll_n = m.forward(xd, ld, normalizeNLL=True, stream=st, **kw)[0].clone()  # (module-owned outputs)
        nll_sn, _ = m.step(xd, ld, normalizeNLL=True, stream=st, **kw)
        st.synchronize()
        assert torch.equal(nll_n, nll_sn)


def test_forward_only_c_entry(s2s):
    """grads = NULL returns 0 under S2S_FORWARD_ONLY (ZERO_GRADS ignored) and an error without it; the flag with
    S2S_BUCKET_EVENTS is an error, not an abort."""
    from s2s_amd import _lib
    lib = _lib.lib
    cfg, x, labels, params = _fwd_case(s2s, "golden_inputs_w16")
    m = s2s.ChorowskiBaseline(cfg, seed=5)
    xd, ld = cu(x), cu(labels, torch.int32)
    B, L, T = xd.shape[0], xd.shape[1], ld.shape[1]
    d, ws = m.dims(B, L, T), m.workspace(B, L, T)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def call(grads, flags):
        rc = lib.s2s_model_step(m.ctx.handle, s2s.nn.stream_ptr(), ctypes.byref(d), p(m.params), p(grads), p(xd),
                                p(ld), 1.0, flags, None, None, p(ws), ws.numel())
        torch.cuda.synchronize()
        return rc

    m.grads.fill_(-3.5)
    assert call(None, _lib.S2S_FORWARD_ONLY | _lib.S2S_ZERO_GRADS) == 0
    assert call(m.grads, _lib.S2S_FORWARD_ONLY | _lib.S2S_ZERO_GRADS) == 0
    assert bool((m.grads == -3.5).all())
    assert call(None, 0) != 0 and b"null gradients" in lib.s2s_last_error()
    assert call(m.grads, _lib.S2S_FORWARD_ONLY | _lib.S2S_BUCKET_EVENTS) != 0
    assert b"S2S_BUCKET_EVENTS" in lib.s2s_last_error()
    assert bool((m.grads == -3.5).all())


# --------------------------------------------------------------------------- Evaluate

EVAL_KW = dict(inputFrameSize=12, hiddenFrameSize=16, outputFrameSize=16, scoreDepth=32, stateDepth=32, outputDepth=11,
               mlpDepth=4, maxoutWindow=3, numLayers=2)
EVAL_SEED = 3


def _eval_case(s2s):
    if "eval" in _cache:
        return _cache["eval"]
    cfg = orc.ModelConfig(**EVAL_KW)
    model = s2s.ChorowskiBaseline(s2s.ModelConfig(**EVAL_KW), seed=EVAL_SEED)
    with torch.no_grad():
        v = model.views()
        for n in ("Wo", "Wy", "Wm", "we"):
            v[n].mul_(3.0)
    P = orc.unflatten(model.params.cpu().double().numpy(), cfg)
    rng = np.random.default_rng(EVAL_SEED)
    eos, Ls, Ts = 4, [23, 9, 31, 16, 12], [5, 3, 7, 4, 6]
    xs = [_f32(rng.standard_normal((L, cfg.inputFrameSize))) for L in Ls]
    ys = []
    for T in Ts:
        y = rng.integers(0, cfg.outputDepth - 1, T)
        y[y >= eos] += 1  # no eos inside
        y[-1] = eos
        ys.append(y.astype(np.int64))
    ref = []
    for x, y in zip(xs, ys):
        _, _, logp, enc = orc.training_step(x[None], y[None], P, cfg, normalizeNLL=False)
        logp, enc = logp[0], enc[0]
        ref.append(dict(nll=-logp[np.arange(len(y)), y].sum(), correct=int((logp.argmax(1) == y).sum()), enc=enc,
                        beam=orc.beam_search(enc, P, cfg, eos, 5, maxseqlength=len(x))))
    _cache["eval"] = (model, cfg, P, xs, ys, eos, ref)
    return _cache["eval"]


@pytest.mark.parametrize("token_map", [False, True])
def test_evaluate_matches_the_oracle(s2s, token_map):
    """Five utterances of different L and T in batches of 2 (sorted by length, so the input order is permuted):
    numCorrect as an integer count and the per-utterance nll (1e-4 relative) against the oracle's whole-model
    forward, predictions under the near-tie rule, PER = the oracle's WagnerFischer on the device's own predictions,
    exactly; with a token_map both sequences are mapped first."""
    model, cfg, P, xs, ys, eos, ref = _eval_case(s2s)
    tmap = (np.arange(cfg.outputDepth) // 2) if token_map else None
    acc, nll, per, preds = model.Evaluate([cu(x) for x in xs], [torch.tensor(y) for y in ys], K=5, max_batch=2,
                                          token_map=tmap)
    det, N = model.eval_detail, len(xs)
    assert det["numCorrect"] == [r["correct"] for r in ref]
    assert acc == sum(r["correct"] for r in ref) / sum(len(y) for y in ys)
    for i, r in enumerate(ref):
        assert abs(det["nll"][i] - r["nll"]) <= TOL * abs(r["nll"]), (i, det["nll"][i], r["nll"])
    assert nll == sum(det["nll"]) / N
    agree, pers = 0, []
    for i, r in enumerate(ref):
        seq = preds[i].tolist()
        assert seq[-1] == eos or len(seq) == len(xs[i]) + 1
        mine = _rescore(r["enc"], seq, P, cfg)
        assert abs(mine - det["score"][i]) <= TOL * max(1.0, abs(mine)), (i, mine, det["score"][i])
        if seq == list(r["beam"][0]):
            agree += 1
        else:
            assert abs(mine - r["beam"][1]) <= TOL * max(1.0, abs(r["beam"][1])), (i, seq, r["beam"])
        a, b = (seq, ys[i].tolist()) if tmap is None else ([int(tmap[t]) for t in seq], [int(tmap[t]) for t in ys[i]])
        dist = orc.wagner_fischer(a, b)
        assert det["dist"][i] == dist, (i, det["dist"][i], dist)
        pers.append(dist / len(ys[i]))
    assert agree >= N - 1
    assert per == sum(pers) / N
    assert model.train  # the mode it was called in is restored


def test_evaluate_refuses_mixed_last_labels(s2s):
    model, cfg, P, xs, ys, eos, ref = _eval_case(s2s)
    bad = [torch.tensor(y) for y in ys]
    bad[2] = bad[2].clone()
    bad[2][-1] = eos + 1
    with pytest.raises(ValueError, match="eos"):
        model.Evaluate([cu(x) for x in xs], bad)
    with pytest.raises(ValueError, match="eos"):
        model.Evaluate([cu(x) for x in xs], [torch.tensor(y) for y in ys], eos=eos + 1)
