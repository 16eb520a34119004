"""Cases, data, references and the checker of the attention-decoder tests (pure NumPy; importable without a GPU).

tests/test_gpu_dec.py runs every case of CASES through nn.Attention on the GPU, four launches ("legs") on the same
module, and compares logp, alpha, dh and every parameter gradient with the float64 oracle (oracle/s2s_oracle.py
attention_fwd / attention_bwd, per utterance on its unpadded slice where there are lengths);
tests/test_dec_case_cpu.py checks, without a GPU, that the cases are what the GPU test takes them for: the expected
route columns follow the dispatch rules, the peaked data really is peaked, the float32 floor of every tensor makes
the bar the tight one, another float32 summation order stays well inside it, and the checker rejects planted faults.

The expected route of a case (`path`, `plan`, `fold`) is written down here by hand from reading dec_xcd_plan,
dec_persist_variant and dec_route (csrc/attn_layout.inc); it is never read back from the library.  The rules:

    Scp     = scoreDepth rounded up to 16 (the module pads the score channels with zeros)
    XCD-local plan (auto mode only; mode = step / persist switch it off):
        widths  LSTM decoder: hybrid with kW = 5 at S = 400, A = 256, Scp = 160          -> XCD_LSTM
                GRU decoder, content attention only: (S, A, Scp) = (256, 512, 512) or (64, 128, 128) -> XCD
                (hybrid attention with the GRU decoder is declined at every width)
        U       = ceil(B / 8) utterances per chain; declined when U > 16, or U > 4 on XCD_LSTM
        nchains = ceil(B / U);  nmax = min(16, 32 // U) chunks per utterance
        XLC     = ceil(L / nmax) rounded up to 4;  NCH = ceil(L / XLC);  declined when XLC > 64 or T > 256
        res     = 2 (resident chunks) while XLC <= 32, else 1 (streamed); S2S_DEC_STREAM = "1" / "0" force 1 / 0;
                  XCD_LSTM is declined unless res = 2
        dec.r4  = 1 on XCD while U <= 4 (the 4-row products), always 1 on XCD_LSTM
    persistent kernels, where the plan declined: mode != step, GRU, content attention, no lengths,
        ceil(L / 16) <= 256 and (S, A, Scp) one of the two GRU width sets -> PERSIST (the launch finds its
        128 workgroups per 16-row tile co-resident for B <= 32); dec.persist_res = 0 when 16 ceil(L / 16) > 128
    everything else: the per-step launches (STEPS), which fold F4 + F5 / K4 + K5 (`fold`) for the LSTM decoder and
        for hybrid attention.

Data.  `plain` draws the parameters U(+-1/sqrt(fan_in)) (hybU x 4 where hybrid is on) and h ~ 0.5 N(0, 1): the
scores of an utterance then span less than 1, alpha ~ 1/L, and the chunk-partial softmax combine, the hybrid halo at
chunk edges, the location carry of the backward and the MonotonicAlignment statistic all run on near-constant
data.  `peaked` scales we, V and Ws (PEAK) and draws h ~ N(0, 1), with the case's seed chosen by a CPU search so
that in the float64 reference (test_dec_case_cpu.py asserts it, on leg 0): (a) max_l alpha > 0.9 on at least half of
the live (b, t); (b) over all (b, t) the chunk holding the argmax (16 frames, XLC frames on the XCD routes)
includes the first chunk and the last, ragged one; (c) for at least one utterance the argmax changes chunk between
two consecutive steps; and max e - min e <= 80 over an utterance's frames, so that no live alpha underflows.

Bar, the rule and constants of tests/rnn_case.py: min(16 x floor, 1e-4 max|ref|) per tensor, the floor being the
largest error of the oracle's own float32 restatements of that tensor on that case and leg (restatements():
BLAS products and rnn_case.ChunkedK products), measured on the references only; an exactly-zero reference at 1e-7.
The XCD routes and the per-step fold reassociate more than a summation order (Wx' = W_g Wd_c Wc, the product-form
scores, the VBAR reference point); measured once on an MI355X, no tensor of any route needed a restatement of
those (largest err / floor 10.9, profiles/dec_case/ratios.txt), so the floor has none.  Discrete decisions -- the
Maxout winners and the MonotonicAlignment indicators -- must equal the float64 reference's wherever its margin
clears the noise and are adopted elsewhere (check_all); the seeds keep at most 1 % of a case's Maxout decisions
and 10 % of its indicator decisions inside the margins, which is why every case with the penalty on is a peaked
one: on plain data the statistic sits within 1e-4 of zero on up to 12 of 15 steps.

Legs, on the same module object: 0 the case's shape; 1 other data with every weight halved, L - 3 and T + 2 (and
other lengths where the case has lengths: a case without lengths stays without, or the persistent route would
become the per-step one); 2 leg 0's data with its last step cut off (T - 1); 3 leg 0 again, exactly.
"""
import collections
import contextlib
import functools

import numpy as np

from oracle import s2s_oracle as orc
from rnn_case import ATOL_ZERO, FLOOR_FACTOR, PREFILL, RTOL, SCALE, _DropTerm, _cast

STEPS, PERSIST, XCD, XCD_LSTM = 0, 1, 2, 3  # tests/paths.py
MAXOUT_MARGIN = 1e-5   # a Maxout decision is clear when u_(1) - u_(2) > MAXOUT_MARGIN max|u|
MONO_MARGIN = 1e-4     # a MonotonicAlignment decision is clear when |stat| > MONO_MARGIN (tests/test_gpu_parity.py)
MAXOUT_CAP, MONO_CAP = 0.01, 0.10  # largest share of a case's decisions inside the margins (float64 reference)
PEAK = {"we": 16.0, "V": 2.0, "Ws": 8.0}
DROPOUT_P = 0.5
NLEGS = 4

Case = collections.namedtuple(
    "Case", "cell B L T A Sc S O M K pen kW nF dropout lengths mode stream data path plan fold note seed "
            "persist_res loose")

SMALL = dict(A=32, Sc=48, S=32)       # no persistent or XCD-local instantiation
MID = dict(A=128, Sc=128, S=64, K=7)
BIG = dict(A=512, Sc=512, S=256, M=8, K=7, O=62)
TIMIT = dict(cell="lstm", A=256, Sc=150, S=400, kW=5, nF=16)  # timit/timit.lua:127-155, scoreDepth 150 run as 160


def C(B, L, T, path, note, plan=None, fold=0, cell="gru", O=11, M=4, K=3, pen=0.0, kW=0, nF=0, dropout=0.0,
      lengths="none", mode="auto", stream=None, data="plain", seed=1, persist_res=None, loose=(), **w):
    return Case(cell, B, L, T, w["A"], w["Sc"], w["S"], O, M, K, pen, kW, nF, dropout, lengths, mode, stream, data,
                path, plan, fold, note, seed, persist_res, tuple(loose))


# plan: (U, nchains, XLC, NCH, res) on the XCD routes.  persist_res: dec.persist_res where the table pins it.
# loose: tensors whose float32 floor may not be 16 x under 1e-4 max|ref| (the note says why); every other is.
CASES = (
    # ---- per-step route, widths with no instantiation
    C(3, 37, 6, STEPS, "GRU content; the plain twin of the next case", seed=144, **SMALL),
    C(3, 37, 6, STEPS, "GRU content, peaked", data="peaked", seed=144, **SMALL),
    C(3, 37, 6, STEPS, "GRU hybrid kW = 5, peaked, penalty on; the sharp softmax amplifies the float32 rounding of "
      "the scores: the floor of four gradients is 0.7e-5 .. 1.5e-5 of max|ref|, so their bar is the 1e-4 one", fold=1,
      kW=5, nF=6, pen=0.3, data="peaked", seed=87, loose=("dWc", "dWd", "ddec.Wh", "dhybW"), **SMALL),
    C(17, 17, 3, STEPS, "GRU hybrid kW = 4 (even: pads 2 left, 1 right); B = 17, L = 17, O = 65; ragged", fold=1,
      kW=4, nF=3, O=65, lengths="ragged", **SMALL),
    C(2, 20, 4, STEPS, "GRU hybrid kW = 1 (no halo)", fold=1, kW=1, nF=4, O=9, **SMALL),
    C(5, 33, 5, STEPS, "GRU hybrid kW = 8 (kMaxHybK: pads 4 left, 3 right); ragged, one L_b = 7 < kW", fold=1,
      kW=8, nF=5, lengths="ragged", **SMALL),
    C(5, 1, 3, STEPS, "LSTM content; L = 1; scoreDepth 20 padded to 32", fold=1, cell="lstm", A=32, Sc=20, S=32),
    C(4, 30, 1, STEPS, "LSTM hybrid kW = 5; T = 1", fold=1, cell="lstm", kW=5, nF=6, **SMALL),
    C(7, 37, 5, STEPS, "GRU content, peaked, ragged, penalty on", pen=0.25, lengths="ragged", data="peaked",
      seed=91, **SMALL),
    C(5, 37, 5, STEPS, "LSTM hybrid kW = 5, peaked, ragged, penalty on", fold=1, cell="lstm", kW=5, nF=6, pen=0.3,
      lengths="ragged", data="peaked", seed=169, **SMALL),
    # ---- per-step route at instantiated widths
    C(5, 37, 4, STEPS, "GRU hybrid at the small instantiated widths: the plan declines hybrid", fold=1, kW=5, nF=8,
      O=29, **MID),
    C(5, 37, 4, STEPS, "mode = step at the small instantiated widths, peaked, penalty on", mode="step", pen=0.3,
      O=29, data="peaked", seed=18, **MID),
    C(5, 37, 4, STEPS, "mode = persist with lengths: dec_persist_variant returns 0, the steps run", mode="persist",
      lengths="ragged", O=29, **MID),
    C(33, 20, 3, STEPS, "LSTM hybrid at the conv + BiLSTM widths with B = 33: U = 5 > 4, steps with the fold",
      fold=1, **TIMIT),
    # ---- persistent route (mode = persist, no lengths, B <= 32)
    C(5, 50, 5, PERSIST, "small widths, L = 50: the resident candidate; peaked, penalty on", mode="persist", pen=0.3,
      O=29, data="peaked", seed=167, persist_res=1, **MID),
    C(3, 130, 3, PERSIST, "L = 130: 16 ceil(L / 16) = 144 > 128, the non-resident kernels",
      mode="persist", O=29, persist_res=0, **MID),
    C(17, 20, 3, PERSIST, "B = 17: a second row tile of one row", mode="persist", O=29, **MID),
    C(3, 20, 3, PERSIST, "the 256 / 512 / 512 widths", mode="persist", **BIG),
    # ---- XCD route
    C(3, 20, 5, XCD, "U = 1", plan=(1, 3, 4, 5, 2), **MID),
    C(32, 20, 3, XCD, "U = 4: the last B on the 4-row products (dec.r4 = 1)", plan=(4, 8, 4, 5, 2), O=29, **MID),
    C(33, 37, 3, XCD, "U = 5: dec.r4 = 0, a last chain of 3 utterances, a last chunk of 5 frames",
      plan=(5, 7, 8, 5, 2), O=29, **MID),
    C(5, 21, 6, XCD, "a ragged last chunk of one frame (XLC = 4, NCH = 6); peaked", plan=(1, 5, 4, 6, 2), O=29,
      data="peaked", seed=6, **MID),
    C(9, 50, 4, XCD, "S2S_DEC_STREAM = 1: Vh-only residency", plan=(2, 5, 4, 13, 1), stream="1", O=29, **MID),
    C(9, 50, 4, XCD, "S2S_DEC_STREAM = 0: no residency", plan=(2, 5, 4, 13, 0), stream="0", O=29, **MID),
    C(128, 70, 3, XCD, "naturally streamed: U = 16, XLC = 36 > 32", plan=(16, 8, 36, 2, 1), O=29, **MID),
    C(9, 50, 5, XCD, "ragged lengths, penalty on, peaked", plan=(2, 5, 4, 13, 2), pen=0.2, lengths="ragged", O=29,
      data="peaked", seed=40, **MID),
    C(3, 20, 3, XCD, "the 256 / 512 / 512 widths", plan=(1, 3, 4, 5, 2), **BIG),
    # ---- XCD-local LSTM route, fused MaxoutMLP
    C(5, 20, 4, XCD_LSTM, "U = 1", plan=(1, 5, 4, 5, 2), **TIMIT),
    C(8, 23, 6, XCD_LSTM, "U = 1, ragged, penalty on, peaked; last chunk of three frames", plan=(1, 8, 4, 6, 2),
      pen=0.3, lengths="ragged", data="peaked", seed=2, **TIMIT),
    C(9, 20, 3, XCD_LSTM, "U = 2, a last chain of one utterance", plan=(2, 5, 4, 5, 2), **TIMIT),
    C(9, 20, 3, XCD_LSTM, "U = 2, ragged", plan=(2, 5, 4, 5, 2), lengths="ragged", **TIMIT),
    # ---- dropout with injected masks, p = 0.5
    C(3, 20, 4, STEPS, "dropout, per-step GRU", dropout=DROPOUT_P, **SMALL),
    C(3, 20, 4, STEPS, "dropout, per-step LSTM hybrid", fold=1, cell="lstm", kW=5, nF=6, dropout=DROPOUT_P, **SMALL),
    C(3, 20, 4, PERSIST, "dropout, persistent route", mode="persist", dropout=DROPOUT_P, O=29, persist_res=1, **MID),
    C(5, 20, 4, XCD, "dropout, XCD route, ragged", plan=(1, 5, 4, 5, 2), dropout=DROPOUT_P, lengths="ragged", O=29,
      **MID),
    C(5, 20, 3, XCD_LSTM, "dropout, XCD-local LSTM route", plan=(1, 5, 4, 5, 2), dropout=DROPOUT_P, **TIMIT),
)


def case_id(c):
    s = f"{c.cell}-{c.B}x{c.L}x{c.T}-{c.A}.{c.Sc}.{c.S}-O{c.O}"
    s += f"-hyb{c.kW}" if c.nF else ""
    s += "-pen" if c.pen else ""
    s += "-drop" if c.dropout else ""
    s += "-ragged" if c.lengths == "ragged" else ""
    s += f"-{c.mode}" if c.mode != "auto" else ""
    s += f"-stream{c.stream}" if c.stream is not None else ""
    s += "-peaked" if c.data == "peaked" else ""
    return s


def leg_shape(c, leg):
    """(L, T) of a leg."""
    if leg == 1:
        return max(1, c.L - 3), c.T + 2
    if leg == 2:
        return c.L, max(1, c.T - 1)
    return c.L, c.T


def chunk_frames(c, L):
    """Frames per attention chunk on the case's route at length L."""
    r = route(c, L, c.T)
    return r[1][2] if r[1] else 16


def route(c, L=None, T=None):
    """The dispatch rules of the module docstring restated: (path, plan or None, fold) of case c's widths, features,
    mode and stream knob at (L, T) -- leg 0's by default.  test_dec_case_cpu.py holds it to the hand-written
    columns on leg 0; the GPU test uses it for the other legs' shapes."""
    L = c.L if L is None else L
    T = c.T if T is None else T
    scp = (c.Sc + 15) // 16 * 16
    lstm, hyb = c.cell == "lstm", c.nF > 0
    gru_widths = (c.S, c.A, scp) in ((256, 512, 512), (64, 128, 128))
    var = 0
    if c.mode == "auto":
        if lstm:
            var = 3 if hyb and c.kW == 5 and (c.S, c.A, scp) == (400, 256, 160) else 0
        elif not hyb and gru_widths:
            var = 1 if c.S == 256 else 2
    plan = None
    if var:
        U = -(-c.B // 8)
        if U <= 16 and not (var == 3 and U > 4):
            nmax = min(16, 32 // U)
            xlc = (-(-L // nmax) + 3) // 4 * 4
            if xlc <= 64 and T <= 256:
                res = 2 if xlc <= 32 else 1
                res = {"1": 1, "0": 0}.get(c.stream, res)
                if not (var == 3 and res != 2):
                    plan = (U, -(-c.B // U), xlc, -(-L // xlc), res)
    if plan:
        return (XCD_LSTM if var == 3 else XCD), plan, 0
    if c.mode != "step" and not hyb and not lstm and c.lengths == "none" and -(-L // 16) <= 256 and gru_widths \
            and c.B <= 32:
        return PERSIST, None, 0
    return STEPS, None, int(lstm or hyb)


# --------------------------------------------------------------------------- data

def _cfg(c):
    return orc.ModelConfig(inputFrameSize=8, hiddenFrameSize=16, outputFrameSize=c.A // 2, scoreDepth=c.Sc,
                           stateDepth=c.S, outputDepth=c.O, mlpDepth=c.M, maxoutWindow=c.K, penalty=c.pen,
                           numLayers=1, hybridAttendFilterSize=c.kW if c.nF else 0, hybridAttendFeatureMaps=c.nF,
                           decoderLSTM=c.cell == "lstm")


def param_names(c):
    """The oracle's parameter names of case c, in the order of the reference's tensors."""
    n = ["V", "Ws", "bs", "we", "Wy", "by", "Wc", "bc", "Wd", "bd"]
    if c.cell == "gru":
        n += ["dec.Wz", "dec.Wr", "dec.Wh"]
    else:
        n += [f"dec.{p}{q}{s}" for q in "ifgo" for p, s in (("W", "x"), ("b", "x"), ("W", "h"), ("b", "h"))]
    n += ["Wm", "bm", "Wo", "bo"]
    if c.nF:
        n += ["hybW", "hybb", "hybU"]
    return n


def _params(c, rng):
    """U(+-1/sqrt(fan_in)) as tests/test_frontend.py _timit_lstm_dec_case draws them, hybU x 4 (the location
    features visibly steer the scores), the peaked scales on top; float32 numbers."""
    S, A, Sc, O, Mk = c.S, c.A, c.Sc, c.O, c.M * c.K

    def u(shape, fan):
        return (rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan)).astype(np.float32)
    P = {"V": u((Sc, A), A), "Ws": u((Sc, S), S), "bs": u(Sc, S), "we": u((1, Sc), Sc), "Wy": u((S, O), O),
         "by": u(S, O), "Wc": u((S, A), A), "bc": u(S, A), "Wd": u((S, 2 * S), 2 * S), "bd": u(S, 2 * S)}
    if c.cell == "gru":
        for g in "zrh":
            P[f"dec.W{g}"] = u((S, 2 * S), 2 * S)
    else:
        for q in "ifgo":
            P[f"dec.W{q}x"], P[f"dec.b{q}x"] = u((S, S), S), u(S, S)
            P[f"dec.W{q}h"], P[f"dec.b{q}h"] = u((S, S), S), u(S, S)
    P.update({"Wm": u((Mk, S + A), S + A), "bm": u(Mk, S + A), "Wo": u((O, c.M), c.M), "bo": u(O, c.M)})
    if c.nF:
        P.update({"hybW": u((c.nF, c.kW), c.kW), "hybb": u(c.nF, c.kW),
                  "hybU": u((Sc, c.nF), c.nF) * np.float32(4.0)})
    if c.data == "peaked":
        for k, s in PEAK.items():
            P[k] = P[k] * np.float32(s)
    return {k: P[k] for k in param_names(c)}


def ragged_lengths(c, L, T, rng):
    """Frame lengths in [1, L] holding L (twice from B = 6), 16, 17, 1 and one L_b < kW where B and L allow; label
    lengths in [1, T] holding T and 1."""
    B = c.B
    flen = rng.integers(1, L + 1, B)
    tlen = rng.integers(1, T + 1, B)
    if B >= 3 and L >= 16:
        flen[1] = 16
    if B >= 4 and L >= 17:
        flen[2] = 17
    if B >= 5 and c.kW > 1:
        flen[3] = min(c.kW - 1, L)
    if B >= 6:
        flen[5] = L
    flen[0], flen[-1] = L, 1
    tlen[0] = T
    tlen[1 % B] = 1
    return flen, tlen


Data = collections.namedtuple("Data", "case leg L T P h labels dlogp flen tlen mask")


@functools.lru_cache(maxsize=None)
def build(c, leg=0):
    """The inputs of case c's leg (module docstring).  Every value is a float32 number (the GPU and the float64
    oracle see the same values); with lengths the padding frames of h hold finite garbage at 3 x scale, the padding
    labels any valid class, and dlogp is zero on padding steps (the loss's seed there).  Arrays are read-only."""
    if leg == 3:
        return build(c, 0)._replace(leg=3)
    L, T = leg_shape(c, leg)
    if leg == 2:
        d = build(c, 0)
        tlen = None if d.tlen is None else np.minimum(d.tlen, T)
        dlogp = d.dlogp[:, :T].copy()
        if tlen is not None:
            dlogp[np.arange(T)[None, :] >= tlen[:, None]] = 0.0
        dlogp.setflags(write=False)
        return d._replace(leg=2, T=T, labels=d.labels[:, :T], dlogp=dlogp, tlen=tlen,
                          mask=None if d.mask is None else d.mask[:, :T])
    P = _params(c, np.random.default_rng(c.seed))
    if leg == 1:
        P = {k: v * np.float32(0.5) for k, v in P.items()}
    rng = np.random.default_rng(c.seed * 7919 + 104729 * (leg + 1))
    hs = 1.0 if c.data == "peaked" else 0.5
    h = (rng.standard_normal((c.B, L, c.A)) * hs).astype(np.float32)
    labels = rng.integers(0, c.O, (c.B, T)).astype(np.int32)
    dlogp = rng.standard_normal((c.B, T, c.O)).astype(np.float32)
    flen = tlen = None
    if c.lengths == "ragged":
        flen, tlen = ragged_lengths(c, L, T, rng)
        h[np.arange(L)[None, :] >= flen[:, None]] *= np.float32(3.0)
        dlogp[np.arange(T)[None, :] >= tlen[:, None]] = 0.0
    mask = None
    if c.dropout:
        mask = ((rng.random((c.B, T, c.S + c.A)) >= c.dropout) / (1.0 - c.dropout)).astype(np.float32)
    for a in (h, labels, dlogp, mask) + tuple(P.values()):
        if a is not None:
            a.setflags(write=False)
    return Data(c, leg, L, T, P, h, labels, dlogp, flen, tlen, mask)


# --------------------------------------------------------------------------- references

FAULTS = ("overwritten", "scale_ignored", "term_missing", "label_shift", "chunk_max_first", "halo_off_by_one",
          "softmax_over_L", "steps_past_Tb", "row16_from_15", "mask_unscaled")


def fault_applies(c, fault, leg=0):
    d = build(c, leg)
    if fault == "term_missing":  # (step 0 has s_{-1} = 0; a single frame has alpha = 1 and de = 0)
        return d.T >= 2 and d.L >= 2
    if fault == "label_shift":  # (step 0 has no previous label)
        return d.T >= 2
    if fault == "chunk_max_first":
        return c.data == "peaked"
    if fault == "halo_off_by_one":
        return c.nF > 0 and d.T >= 2 and d.L >= 2
    if fault == "softmax_over_L":
        return d.flen is not None and bool((d.flen < d.L).any())
    if fault == "steps_past_Tb":  # with dlogp zero on padding steps only the penalty's gradient lives there
        return d.tlen is not None and c.pen > 0 and bool((d.tlen < d.T).any())
    if fault == "row16_from_15":
        return c.B >= 17
    if fault == "mask_unscaled":
        return c.dropout > 0
    return True


@contextlib.contextmanager
def _halo_shifted():
    """Planted fault: the location features read alpha_{t-1} one frame late."""
    real = orc.hybrid_features

    def shifted(alpha_prev, P, kW):
        return real(np.concatenate([np.zeros_like(alpha_prev[:, :1]), alpha_prev[:, :-1]], 1), P, kW)
    orc.hybrid_features = shifted
    try:
        yield
    finally:
        orc.hybrid_features = real


def _chunk_max_first(alpha, chunk):
    """Planted fault: the softmax combined with the first chunk's maximum -- alpha renormalised with the frames whose
    score exceeds chunk 0's maximum clamped to it (log alpha is the score up to a constant per row)."""
    with np.errstate(divide="ignore"):
        la = np.log(alpha)
    la = np.minimum(la, la[..., :chunk].max(-1, keepdims=True))
    e = np.exp(la - la.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


Ref = collections.namedtuple("Ref", "tensors lpad tpad winners margin umax ind stat")
Adopt = collections.namedtuple("Adopt", "winners ind")


def _reference(c, leg, dtype, chunked, fault, adopt, ctx=False):
    d = build(c, leg)
    cfg = _cfg(c)
    B, L, T = c.B, d.L, d.T
    flen = d.flen if d.flen is not None else np.full(B, L)
    tlen = d.tlen if d.tlen is not None else np.full(B, T)
    P = {k: _cast(v, dtype, chunked) for k, v in d.P.items()}
    G = {k: np.full(v.shape, PREFILL, dtype) for k, v in d.P.items()}
    if fault == "term_missing":
        G = _DropTerm(G, "Ws", 1)
    scale = 1.0 if fault == "scale_ignored" else SCALE
    labels = d.labels
    if fault == "label_shift":  # y_prev of step t from labels[t]
        labels = labels.copy()
        labels[:, :-1] = d.labels[:, 1:]
    mask = None
    if d.mask is not None:
        mask = _cast(d.mask * np.float32(1.0 - c.dropout) if fault == "mask_unscaled" else d.mask, dtype, chunked)
    h, dlogp = _cast(d.h, dtype, chunked), _cast(d.dlogp, dtype, chunked)
    logp = np.zeros((B, T, c.O), dtype)
    alpha = np.zeros((B, T, L), dtype)
    dh = np.zeros((B, L, c.A), dtype)
    winners = np.zeros((B, T, c.M), np.int64)
    margin = np.full((B, T, c.M), np.inf)
    ind, stat = np.zeros((B, T)), np.zeros((B, T))
    umax = 0.0
    if d.flen is None:
        groups = [(slice(0, B), L, T)]
    else:
        groups = [(slice(b, b + 1), int(flen[b]), int(tlen[b])) for b in range(B)]
    for rows, n, m in groups:
        if fault == "softmax_over_L":
            n = L
        if fault == "steps_past_Tb":
            m = T
        mk = None if mask is None else mask[rows, :m]
        mo = None if adopt is None else adopt.winners[rows, :m]
        with _halo_shifted() if fault == "halo_off_by_one" else contextlib.nullcontext():
            lref, cache = orc.attention_fwd(h[rows, :n], labels[rows, :m], P, cfg, mk, mo)
            if adopt is not None:
                cache["mono_ind"] = np.asarray(adopt.ind[rows, :m]).astype(dtype)
            dhb = orc.attention_bwd(P, cfg, cache, dlogp[rows, :m], G, scale, mk, softmax_sum_via_context=ctx)
        logp[rows, :m] = np.asarray(lref)
        a = np.asarray(cache["alpha"], np.float64)
        alpha[rows, :m, :n] = a
        dh[rows, :n] = np.asarray(dhb)
        winners[rows, :m] = np.asarray(cache["argmax"])
        u = np.sort(np.asarray(cache["u"], np.float64).reshape(a.shape[0], m, c.M, c.K), -1)
        margin[rows, :m] = u[..., -1] - u[..., -2] if c.K > 1 else np.inf
        umax = max(umax, float(np.abs(u).max()))
        ind[rows, :m] = np.asarray(cache["mono_ind"])
        prev = np.concatenate([np.zeros_like(a[:, :1]), a[:, :-1]], 1)
        stat[rows, :m] = ((n - np.arange(n))[None, None, :] * (a - prev)).sum(-1)
    tensors = {"logp": logp, "alpha": alpha, "dh": dh}
    for k in d.P:
        tensors["d" + k] = np.asarray(G[k])
    if fault == "overwritten":
        tensors["dV"] = tensors["dV"] - PREFILL
    if fault == "row16_from_15":
        tensors["logp"][16] = tensors["logp"][15]
    if fault == "chunk_max_first":
        live = np.arange(T)[None, :] < tlen[:, None]
        for b in range(B):
            nb = int(flen[b])
            alpha[b, live[b], :nb] = _chunk_max_first(alpha[b, live[b], :nb], chunk_frames(c, L))
    lpad = np.arange(L)[None, :] >= flen[:, None]
    tpad = np.arange(T)[None, :] >= tlen[:, None]
    return Ref(tensors, lpad, tpad, winners, margin, umax, ind, stat)


@functools.lru_cache(maxsize=None)
def reference(c, leg=0, dtype=np.float64, chunked=False, fault=None, ctx=False):
    """The oracle's attention_fwd / attention_bwd on case c's leg in `dtype`: {name: tensor} for logp, alpha, dh and
    every parameter gradient `d<name>` (pre-filled with PREFILL, accumulated with SCALE), the padding masks of
    frames and steps, the Maxout winners with their margins u_(1) - u_(2) and max|u|, and the MonotonicAlignment
    indicators with their statistic.  chunked: the float32 restatement with ChunkedK products.  ctx: the softmax
    backward's sum formed from the context, the attention backward kernels' form (sum_j alpha_j d alpha_j = dc . c +
    the carried terms).  fault: one of FAULTS planted (float64).  Leg 3 is leg 0."""
    if leg == 3:
        return reference(c, 0, dtype, chunked, fault, ctx)
    with np.errstate(over="ignore"):
        return _reference(c, leg, dtype, chunked, fault, None, ctx)


def reference_adopting(c, leg, dtype, chunked, adopt, ctx=False):
    """reference() under imposed Maxout winners and MonotonicAlignment indicators (adopt: Adopt(winners (B, T, M),
    ind (B, T))); not cached."""
    with np.errstate(over="ignore"):
        return _reference(c, 0 if leg == 3 else leg, dtype, chunked, None, adopt, ctx)


def restatements(c, leg, adopt=None):
    """The float32 restatements the floor is taken over: plain and ChunkedK.  With a single frame alpha = 1, and the
    oracle's softmax backward alpha (d alpha - sum_j alpha_j d alpha_j) cancels to an exact zero in every precision:
    the score layer's gradients are the prefill, the floor 0.  The attention backward kernels of every route form
    that sum as dc . c + the carried terms (csrc/dec_steps.inc K6), which rounds otherwise than dc . h, so for
    L = 1 that documented form is restated too (measured on lstm-5x1x3: dV, dbs and dwe one to two float32 steps
    of the prefill away from it, against a floor of exactly 0 without this restatement)."""
    L, _ = leg_shape(c, leg)
    if adopt is None:
        rs = [reference(c, leg, np.float32), reference(c, leg, np.float32, True)]
        return rs + [reference(c, leg, np.float32, False, None, True)] if L == 1 else rs
    rs = [reference_adopting(c, leg, np.float32, False, adopt), reference_adopting(c, leg, np.float32, True, adopt)]
    return rs + [reference_adopting(c, leg, np.float32, False, adopt, True)] if L == 1 else rs


def floor_of(name, ref64, rs):
    """max over the restatements of max|restatement - ref64| for tensor `name`."""
    return max(float(np.abs(np.asarray(r.tensors[name], np.float64) - ref64.tensors[name]).max()) for r in rs)


# --------------------------------------------------------------------------- the checker

def check(got, ref64, floor, name):
    """One tensor against the float64 reference at min(16 x floor, 1e-4 max|ref|), the floor measured on the
    references, never on the kernel; an exactly-zero reference at ATOL_ZERO.  Returns (err / floor, None) or
    (err / floor, the failure's message)."""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    if got.shape != ref64.shape:
        return 0.0, f"{name}: shape {got.shape}, expected {ref64.shape}"
    if not np.isfinite(got).all():
        return np.inf, f"{name}: non-finite values"
    scale = float(np.abs(ref64).max())
    err = float(np.abs(got - ref64).max())
    if scale == 0.0:
        print(f"dec {name}: reference is exactly 0, max|got| {err:.3e}")
        ok = err <= ATOL_ZERO
        return 0.0, None if ok else f"{name}: reference is exactly 0, max|got| {err:.3e} > {ATOL_ZERO:.0e}"
    bar = min(FLOOR_FACTOR * floor, RTOL * scale)
    ratio = err / floor if floor > 0 else (0.0 if err == 0 else np.inf)
    print(f"dec {name}: max|got - ref| {err:.3e}, fp32 floor {floor:.3e}, bar {bar:.3e} (max|ref| {scale:.3e}), "
          f"err / floor {ratio:.2f}")
    if err <= bar:
        return ratio, None
    return ratio, f"{name}: max|got - ref| {err:.3e} > bar {bar:.3e} (floor {floor:.3e}, max|ref| {scale:.3e})"


def decision_counts(r):
    """(Maxout decisions, inside the margin, mono decisions, inside the margin) of a float64 reference, live steps."""
    live = ~r.tpad
    nm = int(live.sum()) * r.margin.shape[-1]
    close_m = int(((r.margin <= MAXOUT_MARGIN * r.umax) & live[..., None]).sum())
    return nm, close_m, int(live.sum()), int(((np.abs(r.stat) <= MONO_MARGIN) & live).sum())


def check_all(got, c, leg=0, tag=""):
    """Every tensor of case c's leg through check().  got: {name: array} under the reference's tensor names, plus
    "maxout_argmax" (B, T, M) and "mono_ind" (B, T).  The discrete decisions must equal the float64 reference's
    wherever its margin clears the noise; elsewhere got's are adopted and the references re-run under them.
    alpha and dh past L_b and the indicator past T_b must be exactly zero; logp and alpha on padding steps are not
    specified and not compared.  Returns ({name: err / floor}, [failure messages])."""
    r64 = reference(c, leg)
    name = f"{case_id(c)} leg {leg}{tag}"
    fails = []
    missing = set(r64.tensors) ^ (set(got) - {"maxout_argmax", "mono_ind"})
    assert not missing, sorted(missing)
    live = ~r64.tpad
    win = np.asarray(got["maxout_argmax"]).astype(np.int64)
    gind = np.asarray(got["mono_ind"]).astype(np.float64)
    clear = (r64.margin > MAXOUT_MARGIN * r64.umax) & live[..., None]
    if not np.array_equal(win[clear], r64.winners[clear]):
        n = int((win[clear] != r64.winners[clear]).sum())
        fails.append(f"{name}: {n} Maxout winners differ outside the margin")
    if gind[r64.tpad].any():
        fails.append(f"{name}: MonotonicAlignment indicator set past T_b")
    if c.pen > 0:
        clear = (np.abs(r64.stat) > MONO_MARGIN) & live
        if not np.array_equal(gind[clear], r64.ind[clear]):
            fails.append(f"{name}: MonotonicAlignment decisions differ outside the margin")
    elif gind.any():
        fails.append(f"{name}: MonotonicAlignment indicator set without a penalty")
    adopt = None
    if not np.array_equal(win[live], r64.winners[live]) or not np.array_equal(gind[live], r64.ind[live]):
        w = np.where(live[..., None], win, r64.winners)
        adopt = Adopt(np.clip(w, 0, c.K - 1), np.where(live, gind, 0.0))
        print(f"dec {name}: adopting {int((w != r64.winners).sum())} Maxout winners and "
              f"{int((adopt.ind != r64.ind).sum())} indicators inside the margins")
        r64 = reference_adopting(c, leg, np.float64, False, adopt)
    rs = restatements(c, leg, adopt)
    ratios = {}
    for k in r64.tensors:
        g = np.array(got[k], np.float64)
        if k == "logp":
            g[r64.tpad] = 0.0
        if k == "alpha":
            if g[np.broadcast_to(r64.lpad[:, None, :], g.shape)].any():
                fails.append(f"{name} alpha: non-zero values past L_b")
            g[r64.tpad] = 0.0
        if k == "dh" and g[r64.lpad].any():
            fails.append(f"{name} dh: non-zero values past L_b")
        ratios[k], msg = check(g, r64.tensors[k], floor_of(k, r64, rs), f"{name} {k}")
        if msg:
            fails.append(msg)
    return ratios, fails


def as_got(r):
    """A reference's outputs in the form the GPU test hands to check_all."""
    got = dict(r.tensors)
    got["maxout_argmax"], got["mono_ind"] = r.winners, r.ind
    return got


def peaked_stats(c, leg=0):
    """Of the float64 reference: the share of live (b, t) with max alpha > 0.9, the set of chunks holding an argmax,
    the last chunk's index, whether some utterance's argmax changes chunk between consecutive steps, and the largest
    score span max e - min e of an utterance's frames."""
    r, d = reference(c, leg), build(c, leg)
    a = r.tensors["alpha"]
    live = ~r.tpad
    ch = chunk_frames(c, d.L)
    am = a.argmax(-1) // ch
    moves = any(live[b, t] and live[b, t + 1] and am[b, t] != am[b, t + 1] for b in range(c.B) for t in range(d.T - 1))
    span = 0.0
    for b in range(c.B):
        nb = d.L if d.flen is None else int(d.flen[b])
        la = np.log(a[b, live[b], :nb])
        span = max(span, float((la.max(-1) - la.min(-1)).max()))
    return float((a.max(-1) > 0.9)[live].mean()), set(am[live].tolist()), (d.L - 1) // ch, moves, span
