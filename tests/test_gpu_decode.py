"""The decode path on the device -- Attention:BeamSearch (beam_prep / beam_update / beam_final), WagnerFischer
(edit_distance_kernel) and the LogSoftMax that feeds the search -- at the widths it is used at.

Bookkeeping, exactly: a scripted decoder_mlp ignores its input rows and returns a prescribed table of
log-probabilities (tests/beam_script.py), so the search is a pure function of the table.  Its values lie on a grid
of 1/4, every running score is exact in fp32, and the device must reproduce the float64 restatement token for
token and bit for bit: prediction, score and the complete list of finished hypotheses.  No agreement quota and
no near-tie clause there; the near-tie rule (_check_beam) stays only where the real decoder's fp32
log-probabilities steer the search."""
import ctypes

import numpy as np
import pytest
import torch

import beam_script as bs
from oracle import s2s_oracle as orc

pytestmark = pytest.mark.gpu
RTOL = 1e-4
FLOOR_FACTOR = 16  # the floor rule of tests/test_gpu_fullsize.py


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


# --------------------------------------------------------------------------- scripted search: exact bookkeeping

class ScriptedMLP:
    """decoder_mlp that returns the next count's (B*K, O) rows of a (maxlen + 1, B, K, O) table, whatever its
    input; keeps a copy of every input it was handed (rows[count])."""

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


def _tiny_attention(s2s, O, mlp):
    """S = A = Sc = 16 GRU decoder: its arithmetic is irrelevant under a scripted decoder_mlp."""
    torch.manual_seed(1)
    return s2s.Attention(s2s.GRU(16, 16), mlp, 16, 0, 0, 16, 16, O, True, 0.0).cuda()


def _search(att, h, eos, K, maxlen):
    out = att.BeamSearch(h, eos, K, maxlen, finished=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _assert_exact(table, eos, K, maxlen, got):
    """Every utterance: tokens, length, -1 padding, score (bitwise) and the whole finished list equal the
    reference search's.  Returns the per-utterance traces."""
    toks, lens, scores, nfin, flen, fscore, fseq = got
    B = table.shape[1]
    assert toks.shape == (B, maxlen + 1) and fseq.shape == (B, K, maxlen + 1)
    traces = []
    for b in range(B):
        fin, pred, score, trace = bs.reference_search(table[:, b], eos, K, maxlen)
        traces.append(trace)
        assert int(lens[b]) == len(pred) and toks[b, :lens[b]].tolist() == pred, (b, toks[b].tolist(), pred)
        assert (toks[b, lens[b]:] == -1).all(), (b, toks[b].tolist())
        assert _bits(scores[b]) == _bits(score), (b, float(scores[b]), score)
        assert int(nfin[b]) == len(fin), (b, int(nfin[b]), len(fin))
        for f, (seq, sc) in enumerate(fin):
            assert int(flen[b, f]) == len(seq) and fseq[b, f, :len(seq)].tolist() == seq, \
                (b, f, fseq[b, f, :flen[b, f]].tolist(), seq)
            assert _bits(fscore[b, f]) == _bits(sc), (b, f, float(fscore[b, f]), sc)
    return traces


def _run_scripted(s2s, table, eos, K, maxlen):
    B, O = table.shape[1], table.shape[3]
    att = _tiny_attention(s2s, O, ScriptedMLP(table))
    h = cu(np.random.default_rng(5).standard_normal((B, 4, 16)))
    return _assert_exact(table, eos, K, maxlen, _search(att, h, eos, K, maxlen))


@pytest.mark.parametrize("name", ["stride310", "maxk992", "k1", "k_eq_o", "long300", "maxlen1", "neginf"])
def test_scripted_search_is_exact(s2s, name):
    """The committed tables (beam_script.CASES): 310 and 992 candidates (the arg-max's stride past 256 threads,
    kBeamMaxK), K = 1, K = outputDepth, maxlen = 1, histories and finished sequences past 256 tokens (the history
    copies' stride), and tokens scripted to -inf (never chosen).  tests/test_beam_script_cpu.py asserts, from the
    reference alone, that these tables reach ties at the cut, shared and permuted parents, joint finishes, and
    utterances done between two host polls."""
    K, O, B, maxlen, eos = bs.CASES[name][:5]
    traces = _run_scripted(s2s, bs.case_table(name), eos, K, maxlen)
    if name == "long300":  # the device did copy histories longer than one pass of 256 threads
        assert max(st["count"] for tr in traces for st in tr if st["finished"]) > 257


@pytest.mark.parametrize("name", ["all_equal", "no_eos", "eos_first"])
def test_scripted_search_hand_cases(s2s, name):
    """all_equal: ties everywhere, tokens 0..K-1 in index order.  no_eos: K hypotheses of maxlen + 1 tokens.
    eos_first: K = 1 and eos alone on top at count 0 gives [eos]; the utterance shares its batch with two that run
    to maxlen, and the steps the host keeps issuing until its every-fourth-count poll leave its result untouched."""
    table, eos, K, maxlen = bs.hand_tables()[name]
    B, O = table.shape[1], table.shape[3]
    att = _tiny_attention(s2s, O, ScriptedMLP(table))
    h = cu(np.random.default_rng(5).standard_normal((B, 4, 16)))
    got = _search(att, h, eos, K, maxlen)
    _assert_exact(table, eos, K, maxlen, got)
    toks, lens, scores, nfin, flen, fscore, fseq = got
    if name == "all_equal":
        for b in range(B):
            assert nfin[b] == K and (scores[b] == 0).all()
            assert [fseq[b, f, :maxlen + 1].tolist() for f in range(K)] == [[0] * maxlen + [j] for j in range(K)]
    elif name == "no_eos":
        assert (nfin == K).all() and (flen == maxlen + 1).all() and (lens == maxlen + 1).all()
        assert not (fseq == eos).any()
    else:
        assert len(att.decoder_mlp.rows) == maxlen + 1  # the host stepped on to the last count
        assert lens[0] == 1 and toks[0, 0] == eos and nfin[0] == 1 and flen[0, 0] == 1
        assert _bits(scores[0]) == _bits(-0.25)
        assert (lens[1:] == maxlen + 1).all()


def test_finished_option_leaves_the_default_result_unchanged(s2s):
    """BeamSearch(finished=True) is a diagnostic: the first three results equal the default call's, batched and
    for a single (L, A) utterance."""
    K, O, B, maxlen, eos = bs.CASES["k_eq_o"][:5]
    table = bs.case_table("k_eq_o")
    h = cu(np.random.default_rng(5).standard_normal((B, 4, 16)))
    plain = _tiny_attention(s2s, O, ScriptedMLP(table)).BeamSearch(h, eos, K, maxlen)
    full = _tiny_attention(s2s, O, ScriptedMLP(table)).BeamSearch(h, eos, K, maxlen, finished=True)
    assert len(plain) == 3 and len(full) == 7
    for a, b in zip(plain, full):
        assert torch.equal(a, b)
    one = _tiny_attention(s2s, O, ScriptedMLP(table[:, :1])).BeamSearch(h[0], eos, K, maxlen)
    assert one.tolist() == plain[0][0, :int(plain[1][0])].tolist()


# --------------------------------------------------------------------------- the gathered state is the parent's

def _gru_case(s2s, rng, S, A, Sc, O, hyb, mlp):
    kW, nF = hyb
    torch.manual_seed(3)
    cfg = orc.ModelConfig(inputFrameSize=8, hiddenFrameSize=16, outputFrameSize=A // 2, scoreDepth=Sc, stateDepth=S,
                          outputDepth=O, mlpDepth=4, maxoutWindow=3, numLayers=1, hybridAttendFilterSize=kW,
                          hybridAttendFeatureMaps=nF)
    att = s2s.Attention(s2s.GRU(S, S), mlp, Sc, kW, nF, S, A, O, True, 0.0).cuda()
    if nF:
        with torch.no_grad():
            att.own["hybU"].mul_(4.0)  # location features visibly steer the scores
    P = {n: _np(t) for n, t in att.own.items()}
    P.update({f"dec.W{g}": _np(t) for g, t in zip("zrh", att.decoder_recurrent.weight)})
    return att, cfg, P


@pytest.mark.parametrize("variant", ["gru", "gru_hybrid", "lstm_hybrid"])
def test_gathered_state_is_the_parents(s2s, fe, variant):
    """Attention.lua:400-430: a survivor continues from its parent's hidden {alpha, s, mem}.  The scripted table
    steers the search (shared parents, permuted parents, utterances done early -- asserted from the trace), and
    the [s_t; c_t] row the device hands the decoder_mlp at every count and active row must be the v the float64
    oracle hands its mlp at the corresponding call of the same search: 1e-4 of max|ref| per count.  GRU with
    content attention (s), GRU with hybrid attention (alpha_{t-1} per hypothesis), LSTM with hybrid attention (the
    cell)."""
    from test_frontend import _load_lstm_attention, _lstm_dec_case
    K, O, B, maxlen, eos = bs.CASES["gather"][:5]
    table = bs.case_table("gather")
    rng = np.random.default_rng(11)
    S, A, Sc, L = 32, 64, 48, 24
    mlp = ScriptedMLP(table)
    if variant == "lstm_hybrid":
        cfg, P = _lstm_dec_case(rng, S, A, Sc, O, (5, 16), "maxout")
        att, _ = _load_lstm_attention(s2s, fe, P, cfg, mlp)
    else:
        att, cfg, P = _gru_case(s2s, rng, S, A, Sc, O, (5, 8) if variant == "gru_hybrid" else (0, 0), mlp)
    h = (rng.standard_normal((B, L, A)) * 1.5).astype(np.float32).astype(np.float64)
    traces = _assert_exact(table, eos, K, maxlen, _search(att, cu(h), eos, K, maxlen))
    ev = [bs.events(tr) for tr in traces]
    assert sum(e["shared_parent"] for e in ev) >= 1 and sum(e["parents_out_of_order"] for e in ev) >= 1
    assert len({tr[-1]["count"] for tr in traces}) >= 2  # an utterance done while others continue
    rows = [r.double().cpu().numpy().reshape(B, K, S + A) for r in mlp.rows]
    gpu = {c: [] for c in range(maxlen + 1)}
    ref = {c: [] for c in range(maxlen + 1)}
    for b in range(B):
        script = bs.StatefulScript(table[:, b], [st["active"] for st in traces[b]])
        orc.beam_search(h[b], P, cfg, eos, K, maxlen, mlp=script)
        assert script.n == len(script.calls)
        for (c, r), v in script.seen.items():
            gpu[c].append(rows[c][b, r])
            ref[c].append(v)
    for c in range(maxlen + 1):
        if ref[c]:
            g, r = np.stack(gpu[c]), np.stack(ref[c])
            err = np.abs(g - r).max() / np.abs(r).max()
            assert np.isfinite(g).all() and err <= RTOL, (variant, c, err)


# --------------------------------------------------------------------------- the real decoder, reference widths

def test_beam_search_at_the_reference_decoder_widths(s2s):
    """The fused decoder at the Chorowski baseline's widths (A = Sc = 512, S = 256, O = 62, Maxout 64 x 7): B = 3
    utterances x K = 5 = 15 hypothesis rows (not a multiple of the 16-row tile) and 310 candidates.  The real
    decoder's fp32 log-probabilities steer this search, so it is judged by _check_beam's near-tie rule."""
    from test_frontend import _check_beam
    torch.manual_seed(21)
    rng = np.random.default_rng(21)
    cfg = orc.ModelConfig(numLayers=1)
    S, A, Sc, O, M, Kw = cfg.stateDepth, cfg.annotationDepth, cfg.scoreDepth, cfg.outputDepth, cfg.mlpDepth, \
        cfg.maxoutWindow
    assert (S, A, Sc, O, M, Kw) == (256, 512, 512, 62, 64, 7)
    att = s2s.Attention(s2s.GRU(S, S), s2s.MaxoutMLP(S + A, M, Kw, O), Sc, 0, 0, S, A, O, True, 0.0).cuda()
    P = {n: _np(t) for n, t in att.own.items()}
    P.update({f"dec.W{g}": _np(t) for g, t in zip("zrh", att.decoder_recurrent.weight)})
    P.update({n: _np(t) for n, t in zip(("Wm", "bm", "Wo", "bo"), att.decoder_mlp.weight)})
    h = (rng.standard_normal((3, 40, A)) * 1.5).astype(np.float32).astype(np.float64)
    _check_beam(att, h, P, cfg, 23, 5, 8)


# --------------------------------------------------------------------------- edit distance

def _pad(seqs, width=None):
    width = max(1, max(len(s) for s in seqs)) if width is None else width
    out = np.zeros((len(seqs), width), np.int32)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, np.array([len(s) for s in seqs], np.int32)


def _edit(s2s, A, B, lda=None, ldb=None):
    a, alen = _pad(A, lda)
    b, blen = _pad(B, ldb)
    out = s2s.nn.edit_distance(cu(a, torch.int32), cu(alen, torch.int32), cu(b, torch.int32), cu(blen, torch.int32))
    torch.cuda.synchronize()
    return out.cpu().numpy().tolist()


def test_edit_distance_known_answers(s2s):
    A = [list(b"kitten"), [1, 2, 3, 4], [1, 2, 3], [], [5, 6, 7, 8, 9], [], [4]]
    B = [list(b"sitting"), [1, 2, 3, 4], [4, 5, 6, 7, 8], [9, 9, 9], [], [], [4]]
    want = [3, 0, 5, 3, 5, 0, 0]
    assert [orc.wagner_fischer(a, b) for a, b in zip(A, B)] == want
    assert _edit(s2s, A, B) == want


def test_edit_distance_is_symmetric_with_different_strides(s2s):
    rng = np.random.default_rng(2)
    A = [rng.integers(0, 5, rng.integers(0, 40)).tolist() for _ in range(50)]
    B = [rng.integers(0, 5, rng.integers(0, 23)).tolist() for _ in range(50)]
    ref = [orc.wagner_fischer(a, b) for a, b in zip(A, B)]
    assert _edit(s2s, A, B, 47, 23) == ref  # lda != ldb
    assert _edit(s2s, B, A, 23, 47) == ref


def test_edit_distance_one_pair_and_a_thousand(s2s):
    rng = np.random.default_rng(3)
    assert _edit(s2s, [[1, 2, 3, 4, 5]], [[2, 3, 9, 5]]) == [orc.wagner_fischer([1, 2, 3, 4, 5], [2, 3, 9, 5])]
    # lengths 0 and full (= the row stride) among them
    la, lb = 12, 9
    A = [rng.integers(0, 4, n).tolist() for n in rng.integers(0, la + 1, 1000)]
    B = [rng.integers(0, 4, n).tolist() for n in rng.integers(0, lb + 1, 1000)]
    A[0], B[0], A[1], B[1], A[999], B[999] = [], [], [1] * la, [], [2] * la, [2] * lb
    assert {len(a) for a in A} == set(range(la + 1)) and {len(b) for b in B} == set(range(lb + 1))
    assert _edit(s2s, A, B, la, lb) == [orc.wagner_fischer(a, b) for a, b in zip(A, B)]


def test_edit_distance_extreme_tokens(s2s):
    big = 2 ** 31 - 1
    A = [[-1, -2, big, big - 1, 0], [big, -big - 1, -1], [big - 1] * 4]
    B = [[-1, big, big - 1, 0, -2], [big - 1, -big - 1, 1], [big] * 4]
    assert _edit(s2s, A, B) == [orc.wagner_fischer(a, b) for a, b in zip(A, B)]


def test_edit_distance_long_pair(s2s):
    rng = np.random.default_rng(4)
    a = rng.integers(0, 40, 700).tolist()
    b = list(a)
    for _ in range(150):  # a noisy copy: substitutions, deletions, insertions -> about 650 tokens
        i = int(rng.integers(0, len(b)))
        b[i] = int(rng.integers(0, 40))
    for _ in range(75):
        del b[int(rng.integers(0, len(b)))]
    for _ in range(25):
        b.insert(int(rng.integers(0, len(b))), int(rng.integers(0, 40)))
    assert len(a) == 700 and len(b) == 650
    assert _edit(s2s, [a], [b]) == [orc.wagner_fischer(a, b)]


def test_edit_distance_at_the_row_stride_guard(s2s):
    """lda = 16383 is the guard's edge: (lda + 1) ints = exactly 64 KB of dynamic LDS.  alen = 16383 fills it;
    a second pair uses 3 tokens of the same stride.  lda = 16384 is refused with a message before any launch."""
    rng = np.random.default_rng(6)
    a0 = rng.integers(0, 3, 16383).tolist()
    A, B = [a0, [1, 2, 3]], [[a0[0], 7], [1, 3]]
    assert _edit(s2s, A, B, 16383, 2) == [orc.wagner_fischer(a, b) for a, b in zip(A, B)]
    with pytest.raises(s2s._lib.S2SError, match="edit distance: bad sizes"):
        _edit(s2s, [[1, 2, 3]], [[1, 3]], 16384, 2)
    # the C entry itself: a nonzero code, a message, and the output untouched (no kernel ran)
    lib, dev = s2s._lib.lib, torch.cuda.current_device()
    a, alen = cu(np.ones((1, 16384)), torch.int32), cu([3], torch.int32)
    b, blen = cu(np.ones((1, 2)), torch.int32), cu([2], torch.int32)
    out = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.s2s_edit_distance(s2s.nn.get_context(dev).handle, s2s.nn.stream_ptr(), 1, ptr(a), ptr(alen), 16384,
                               ptr(b), ptr(blen), 2, ptr(out))
    torch.cuda.synchronize()
    assert rc != 0 and b"edit distance" in lib.s2s_last_error() and out.item() == -77


# --------------------------------------------------------------------------- LogSoftMax wider than one wave

def _lsm(x, dy):
    """The kernel's formula in x's precision: y = x - (m + log(sum exp(x - m))), dx = dy - exp(y) sum(dy)."""
    with np.errstate(invalid="ignore"):
        m = x.max(-1, keepdims=True)
        y = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True, dtype=x.dtype)))
        dx = dy - np.exp(y) * dy.sum(-1, keepdims=True, dtype=x.dtype)
    return y, dx


def _check_lsm(fe, x32, dy32, tag):
    mod = fe.LogSoftMax()
    y = mod.forward(cu(x32))
    dx = mod.backward(cu(x32), cu(dy32))
    torch.cuda.synchronize()
    y, dx = y.cpu().numpy().astype(np.float64), dx.cpu().numpy().astype(np.float64)
    y64, dx64 = _lsm(x32.astype(np.float64), dy32.astype(np.float64))
    y32, dx32 = _lsm(x32, dy32)
    fin = np.isfinite(y64)
    assert (y[~fin] == -np.inf).all() and np.isfinite(y[fin]).all() and np.isfinite(dx).all(), tag
    for name, g, r32, r64 in (("y", y[fin], y32[fin], y64[fin]), ("dx", dx, dx32, dx64)):
        scale = np.abs(r64).max()
        err, floor = np.abs(g - r64).max(), np.abs(r32.astype(np.float64) - r64).max()
        bar = min(FLOOR_FACTOR * floor, RTOL * scale)
        print(f"LogSoftMax {tag} {name}: max|gpu - ref| {err:.3e}, fp32 restatement {floor:.3e}, "
              f"bar {bar:.3e} (max|ref| {scale:.3e})")
        assert err <= bar, (tag, name, err, floor, bar)


@pytest.mark.parametrize("n", [1, 29, 62, 64, 65, 200])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1001])
def test_logsoftmax_matches_float64(fe, rows, n):
    """fe.LogSoftMax forward and backward against float64 on the fp32-rounded input, logits scaled x30; n past 64
    takes the kernels' stride over the vocabulary, rows past 4 more than one block.  Bar: 16x the error of the fp32
    NumPy restatement of the same formula on the same input, never above 1e-4 of max|ref|."""
    rng = np.random.default_rng(rows * 1000 + n)
    x = (rng.standard_normal((rows, n)) * 30).astype(np.float32)
    dy = rng.standard_normal((rows, n)).astype(np.float32)
    _check_lsm(fe, x, dy, f"rows {rows} n {n}")


def test_logsoftmax_with_some_minus_inf_entries(fe):
    """-inf logits (tokens ruled out) in some entries of every row: -inf out there, finite gradients, and the other
    entries as if the -inf ones were absent."""
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((5, 100)) * 30).astype(np.float32)
    dy = rng.standard_normal((5, 100)).astype(np.float32)
    mask = rng.random((5, 100)) < 0.3
    mask[:, 0], mask[:, 1] = True, False  # some, not all, in every row
    x[mask] = -np.inf
    _check_lsm(fe, x, dy, "-inf entries")
    # (reference property: a -inf entry adds exp(-inf) = 0 to the row's sum, so the others are as if it were absent)
    y64, _ = _lsm(x.astype(np.float64), dy.astype(np.float64))
    for r in range(5):
        keep = ~mask[r]
        yk, _ = _lsm(x[r, keep].astype(np.float64), dy[r, keep].astype(np.float64))
        np.testing.assert_array_equal(y64[r, keep], yk)
