"""Cases, data, references and the checker of the recurrent-layer tests (pure NumPy; importable without a GPU).

tests/test_gpu_rnn.py runs every case of GRU_CASES / LSTM_CASES through nn.RNN / BiRNN on the GPU and compares
each output tensor with the float64 oracle (oracle/s2s_oracle.py); tests/test_rnn_case_cpu.py checks, without a
GPU, that the cases are what the GPU test takes them for: the expected-path columns follow the dispatch rules,
the float32 floor of every tensor is small enough to make the bar tight, another legitimate float32 summation
order stays well inside the bar, and the checker rejects planted faults.

The expected dispatch of a case (`path`, `fused`) is written down here from reading gru_persist_supported,
gru_persist_fused_xproj, lstm_persist_supported and use_persistent (csrc/gru_persist.hip, lstm_persist.hip,
gru.hip); it is never read back from the library.

    chains  = ndir * ceil(B / 16)         (direction x 16-row tile), dealt 8 per round
    GRU     persistent iff H in {64, 128, 256, 512} and (2H/16) * rounds <= 32 (one workgroup per CU, 32 CUs
            per XCD) -> at most 4 / 2 / 1 rounds at H = 64 / 128 / 256, and never at H = 512
    fused x-projection iff persistent, B <= 64, D % 32 == 0 and the spare slots of the last round,
            (2H/16) * (8 * rounds - chains), are at least 32: 4 spare chains at H = 64, 2 at 128, 1 at 256
    LSTM    persistent iff no peepholes, H in {64, 128, 256} and (H/16) * rounds <= 32
            -> at most 8 / 4 / 2 rounds at H = 64 / 128 / 256
"""
import collections
import functools

import numpy as np

from oracle import s2s_oracle as orc

RTOL = 1e-4        # tests/test_gpu_decode.py's convention: bar = min(FLOOR_FACTOR * floor, RTOL * max|ref|)
FLOOR_FACTOR = 16
ATOL_ZERO = 1e-7   # tests/test_gpu_parity.py assert_rel: an exactly-zero reference has no relative scale
PREFILL = 0.25     # gradWeight before the backward call: gradients accumulate
SCALE = 0.5        # the backward call's scale

Case = collections.namedtuple("Case", "cell B L D H dirn peep data lengths path fused xscale ab note")


def G(B, L, D, H, dirn, lengths, path, fused, note, data="plain", xscale=1.0, ab=False):
    return Case("gru", B, L, D, H, dirn, False, data, lengths, path, fused, xscale, ab, note)


def Lc(B, L, D, H, dirn, lengths, path, note, peep=False, data="plain", xscale=1.0, ab=False):
    return Case("lstm", B, L, D, H, dirn, peep, data, lengths, path, None, xscale, ab, note)


# path: gru.fwd.path = gru.bwd.path; fused: gru.fused_xproj.  Every persistent H fuses at layer level for some D
# (H = 64 needs 4 spare chains, so at most 4 chains: B <= 32 bidirectional); a second round never fuses (more than
# 8 chains means B > 64).  H = 512 has no persistent shape: its cases pin the fall-back.  ab: also run with
# S2S_GRU_MODE=step.
GRU_CASES = (
    # persistent widths
    G(1, 1, 32, 64, "bi", "none", 1, 1, "one utterance, one frame", ab=True),
    G(17, 5, 64, 64, "bi", "ragged", 1, 1, "H = 64, D a multiple of 32; 4 chains, 4 spare: the last B that fuses"),
    G(5, 4, 40, 64, "fwd", "ragged", 1, 0, "H = 64 with D % 32 != 0: the separate x-projection GEMM"),
    G(16, 4, 40, 128, "rev", "ragged", 1, 0, "uni reverse, exactly the ring, unfused x-projection"),
    G(17, 5, 64, 128, "bi", "ragged", 1, 1, "H = 128 fused, just past the ring", ab=True),
    G(33, 9, 96, 256, "bi", "ragged", 1, 1, "H = 256 against float64, three tiles", ab=True),
    G(64, 3, 32, 256, "bi", "none", 1, 0, "the largest supported batch at 256 (8 chains, no spare slot)"),
    G(65, 6, 64, 256, "bi", "ragged", 0, 0, "10 chains at H = 256: the first unsupported, per-step launches"),
    G(128, 3, 32, 256, "bi", "none", 0, 0, "16 chains at H = 256: per-step launches"),
    G(129, 3, 32, 256, "bi", "none", 0, 0, "18 chains at H = 256: per-step launches"),
    G(65, 6, 64, 128, "bi", "ragged", 1, 0, "10 chains at H = 128: the second round; B > 64 never fuses"),
    G(128, 3, 32, 128, "bi", "none", 1, 0, "16 chains at H = 128: the last supported"),
    G(129, 3, 32, 128, "bi", "none", 0, 0, "18 chains at H = 128: the first unsupported"),
    G(65, 4, 32, 64, "bi", "ragged", 1, 0, "10 chains at H = 64: the second round"),
    G(5, 2, 32, 64, "bi", "ragged", 1, 1, "L = 2: below the ring"),
    G(5, 3, 32, 128, "fwd", "ragged", 1, 1, "L = 3: below the ring, uni forward"),
    G(17, 5, 64, 128, "bi", "ragged", 1, 1, "H = 128, saturated gates", data="saturated", xscale=100.0),
    # H = 512: 64 members per chain are more than the 32 CUs of an XCD hold, so every shape takes the per-step launches
    G(17, 9, 64, 512, "bi", "ragged", 0, 0, "H = 512"),
    G(64, 3, 32, 512, "bi", "none", 0, 0, "H = 512, 8 chains"),
    G(65, 3, 32, 512, "fwd", "none", 0, 0, "H = 512, 5 chains"),
    G(65, 3, 32, 512, "bi", "none", 0, 0, "H = 512, 10 chains"),
    G(17, 9, 64, 512, "bi", "ragged", 0, 0, "H = 512, saturated gates", data="saturated", xscale=150.0),
    # per-step widths
    G(17, 7, 20, 16, "bi", "ragged", 0, 0, "H = 16"),
    G(33, 5, 40, 48, "bi", "none", 0, 0, "H = 48, three tiles"),
    G(17, 5, 40, 192, "bi", "none", 0, 0, "a multiple of 64 that is not persistent"),
    G(5, 4, 64, 320, "bi", "none", 0, 0, "H = 320"),
    G(16, 5, 40, 48, "rev", "ragged", 0, 0, "uni reverse with lengths, per-step"),
    G(17, 7, 20, 16, "bi", "ragged", 0, 0, "H = 16, saturated gates", data="saturated", xscale=60.0),
)

# path: lstm.fwd.path = lstm.bwd.path.  ab: also run with S2S_LSTM_MODE=step.
LSTM_CASES = (
    # persistent, no peepholes
    Lc(1, 1, 32, 64, "bi", "none", 1, "one utterance, one frame", ab=True),
    Lc(17, 5, 64, 128, "bi", "ragged", 1, "H = 128", ab=True),
    Lc(33, 9, 96, 256, "bi", "ragged", 1, "H = 256 (launch_fwd_nc<4>, launch_bwd_nc<16>), three tiles", ab=True),
    Lc(65, 4, 32, 256, "bi", "none", 1, "10 chains: the second round"),
    Lc(128, 3, 32, 256, "bi", "none", 1, "16 chains: the last supported"),
    Lc(129, 3, 32, 256, "bi", "none", 0, "18 chains: the first unsupported"),
    Lc(16, 4, 40, 128, "rev", "ragged", 1, "uni reverse with lengths, persistent"),
    Lc(17, 5, 64, 128, "bi", "ragged", 1, "H = 128, saturated gates", data="saturated", xscale=35.0),
    # width 192 and per-step
    Lc(17, 5, 40, 192, "bi", "ragged", 0, "H = 192 has no persistent instantiation: per-step launches"),
    Lc(17, 5, 40, 192, "bi", "none", 0, "H = 192 with peepholes", peep=True),
    Lc(5, 4, 64, 320, "bi", "none", 0, "H = 320"),
    Lc(17, 5, 64, 64, "bi", "ragged", 0, "peepholes at a persistent width", peep=True),
    Lc(33, 4, 32, 256, "bi", "none", 0, "peepholes at H = 256", peep=True),
    Lc(17, 7, 20, 16, "bi", "none", 0, "H = 16"),
    Lc(17, 7, 20, 16, "bi", "ragged", 0, "H = 16 with peepholes", peep=True),
    Lc(16, 4, 40, 64, "rev", "ragged", 0, "uni reverse with lengths, per-step", peep=True),
    Lc(17, 7, 20, 16, "bi", "ragged", 0, "H = 16 with peepholes, saturated gates", peep=True, data="saturated",
       xscale=35.0),
)


def case_id(c):
    return f"{c.B}x{c.L}x{c.D}x{c.H}-{c.dirn}-{c.lengths}" + ("-peep" if c.peep else "") + \
        ("-sat" if c.data == "saturated" else "")


def ndir(c):
    return 2 if c.dirn == "bi" else 1


def reverses(c):
    return {"bi": (False, True), "fwd": (False,), "rev": (True,)}[c.dirn]


def nchains(c):
    return ndir(c) * ((c.B + 15) // 16)


# --------------------------------------------------------------------------- data

def ragged_lengths(B, L, rng):
    """Lengths in [1, L]; utterance 0 has L frames and the last one 1; lengths 4 and 5 both present where B and L
    allow; with more than one 16-row tile, every utterance of the second tile is shorter than L."""
    lens = rng.integers(1, L + 1, B)
    if B >= 4 and L >= 5:
        lens[1], lens[2] = 4, 5
    if B > 16 and L >= 2:
        lens[16:32] = np.minimum(lens[16:32], L - 1)
    lens[0] = L
    lens[-1] = 1
    return lens


LSTM_GATES = orc.LSTM_GATES  # ("i", "f", "g", "o"): the order of nn.LSTM's flat parameter list


def _uniform(rng, shape, stdv):
    return ((rng.random(shape) * 2 - 1) * stdv).astype(np.float32)


def _weights(c, rng):
    """One direction's parameters, drawn as the module's reset draws them (nn.GRU: U(+-1/sqrt(D + H)) for the three
    (H, H + D) matrices; nn.LSTM: U(+-1/sqrt(in)) per Linear, weight and bias), as float32 numbers."""
    D, H = c.D, c.H
    if c.cell == "gru":
        return {k: _uniform(rng, (H, H + D), 1.0 / np.sqrt(D + H)) for k in ("Wz", "Wr", "Wh")}
    P = {}
    sx, sh = 1.0 / np.sqrt(D), 1.0 / np.sqrt(H)
    for q in LSTM_GATES:
        P[f"W{q}x"], P[f"b{q}x"] = _uniform(rng, (H, D), sx), _uniform(rng, (H,), sx)
        P[f"W{q}h"], P[f"b{q}h"] = _uniform(rng, (H, H), sh), _uniform(rng, (H,), sh)
    if c.peep:
        for q in ("i", "f", "o"):
            P[f"W{q}c"], P[f"b{q}c"] = _uniform(rng, (H, H), sh), _uniform(rng, (H,), sh)
    return P


Data = collections.namedtuple("Data", "case leg x dy lens W")


@functools.lru_cache(maxsize=None)
def build(c, leg=0):
    """The inputs of case c: leg 0 is the first launch; leg 1 the relaunch of the same module with another x and dy,
    other lengths (ragged wherever L >= 2, also where leg 0 had none) and the weights of leg 0 halved.  x, dy and
    the weights are float32 numbers (the GPU and the float64 oracle see the same values); x holds finite data on
    padding frames too."""
    seed = (c.B * 1000003 + c.L * 10007 + c.D * 101 + c.H) * 4 + 2 * (c.cell == "lstm") + c.peep
    wrng = np.random.default_rng(seed)
    W = [_weights(c, wrng) for _ in range(ndir(c))]
    if leg:
        W = [{k: v * np.float32(0.5) for k, v in w.items()} for w in W]
    rng = np.random.default_rng(seed + 7919 * (leg + 1))
    x = (rng.standard_normal((c.B, c.L, c.D)) * c.xscale).astype(np.float32)
    dy = rng.standard_normal((c.B, c.L, ndir(c) * c.H)).astype(np.float32)
    lens = None
    if c.lengths == "ragged" or (leg and c.L >= 2):
        lens = ragged_lengths(c.B, c.L, rng)
    for a in (x, dy):
        a.setflags(write=False)
    return Data(c, leg, x, dy, lens, W)


# --------------------------------------------------------------------------- references

class ChunkedK(np.ndarray):
    """A float32 array whose matrix products are summed in K-chunks of 16, the chunks accumulated in order:
    another legitimate fp32 summation order than the BLAS product of the plain float32 restatement.  Every
    result of an operation with a ChunkedK operand is a ChunkedK again, so the oracle's code runs unchanged."""
    CHUNK = 16

    @staticmethod
    def _plain(v):
        if isinstance(v, ChunkedK):
            return v.view(np.ndarray)
        if isinstance(v, (list, tuple)):
            return type(v)(ChunkedK._plain(u) for u in v)
        return v

    @staticmethod
    def _wrap(v):
        return v.view(ChunkedK) if isinstance(v, np.ndarray) else v

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kw):
        ins = [self._plain(i) for i in inputs]
        if ufunc is np.matmul and method == "__call__" and out is None:
            a, b = ins
            K = a.shape[-1]
            acc = a[..., :self.CHUNK] @ b[:self.CHUNK]
            for k in range(self.CHUNK, K, self.CHUNK):
                acc = acc + a[..., k:k + self.CHUNK] @ b[k:k + self.CHUNK]
            return self._wrap(acc)
        if out is not None:
            kw["out"] = tuple(self._plain(o) for o in out)
        res = getattr(ufunc, method)(*ins, **kw)
        if out is not None:
            return out[0] if len(out) == 1 else out
        return self._wrap(res)

    def __array_function__(self, func, types, args, kwargs):
        res = func(*self._plain(args), **{k: self._plain(v) for k, v in kwargs.items()})
        return self._wrap(res)


def _cast(a, dtype, chunked):
    a = np.asarray(a).astype(dtype)
    return a.view(ChunkedK) if chunked else a


def _fwd(c, x, W, rev):
    if c.cell == "gru":
        return orc.gru_seq_fwd(x, W["Wz"], W["Wr"], W["Wh"], rev)
    return orc.lstm_seq_fwd(x, W, rev, c.peep)


def _bwd(c, x, W, sv, dy, grads, rev, scale):
    if c.cell == "gru":
        return orc.gru_seq_bwd(x, W["Wz"], W["Wr"], W["Wh"], sv, dy, grads, rev, scale)[0]
    return orc.lstm_seq_bwd(x, W, sv, dy, grads, rev, c.peep, scale)


class _DropTerm(dict):
    """A gradient dict that loses the n-th `grads[key] += term` (planted fault: one time step's term missing)."""

    def __init__(self, base, key, n):
        super().__init__(base)
        self.key, self.left, self.skipping = key, n, False

    def __getitem__(self, k):
        v = super().__getitem__(k)
        if k == self.key:
            self.left -= 1
            if self.left == 0:
                self.skipping = True
                return v.copy()
        return v

    def __setitem__(self, k, v):
        if k == self.key and self.skipping:
            self.skipping = False
            return
        super().__setitem__(k, v)


FAULTS = ("reverse_from_L", "state_zeroed_at_4", "term_missing", "overwritten", "scale_ignored", "padding_1e-30",
          "row16_from_15")


def fault_applies(c, fault, leg=0):
    d = build(c, leg)
    if fault == "reverse_from_L":  # a reverse direction and an utterance shorter than L
        return d.lens is not None and True in reverses(c) and bool((d.lens < c.L).any())
    if fault == "state_zeroed_at_4":  # utterance 0 has all L frames
        return c.L >= 5
    if fault == "padding_1e-30":
        return d.lens is not None and bool((d.lens < c.L).any())
    if fault == "row16_from_15":
        return c.B >= 17
    return True


def _first_grad_key(c):
    return "Wh" if c.cell == "gru" else "Wgx"


def _preact_max(c, x, W, sv):
    """max |pre-activation| of the sigmoid gates, restated from the saved activations."""
    hp = sv["hprev"]
    if c.cell == "gru":
        hx = np.concatenate([hp, x], axis=-1)
        return max(float(np.abs(hx @ W[k].T).max()) for k in ("Wz", "Wr"))
    m = 0.0
    for q in ("i", "f", "o"):
        a = x @ W[f"W{q}x"].T + W[f"b{q}x"] + hp @ W[f"W{q}h"].T + W[f"b{q}h"]
        if c.peep:
            a = a + (sv["c"] if q == "o" else sv["cprev"]) @ W[f"W{q}c"].T + W[f"b{q}c"]
        m = max(m, float(np.abs(a).max()))
    return m


Ref = collections.namedtuple("Ref", "tensors pad sat_fraction preact_max")


def _reference(c, leg, dtype, chunked, fault):
    d = build(c, leg)
    B, L, H = c.B, c.L, c.H
    lens = d.lens if d.lens is not None else np.full(B, L)
    x = _cast(d.x, dtype, chunked)
    dy = _cast(d.dy, dtype, chunked)
    scale = 1.0 if fault == "scale_ignored" else SCALE
    T = {}
    dx = np.zeros((B, L, c.D), dtype)
    gates, amax, planted = [], 0.0, False
    # one oracle call for the whole batch without lengths; one per utterance, on its unpadded slice, with them
    groups = [(slice(0, B), L)] if d.lens is None else [(slice(b, b + 1), int(lens[b])) for b in range(B)]
    for i, rev in enumerate(reverses(c)):
        W = {k: _cast(v, dtype, chunked) for k, v in d.W[i].items()}
        grads = {k: np.full(v.shape, PREFILL, dtype) for k, v in d.W[i].items()}
        if fault == "term_missing" and i == 0:
            grads = _DropTerm(grads, _first_grad_key(c), 1)
        y = np.zeros((B, L, H), dtype)
        for gi, (rows, n) in enumerate(groups):
            xb = x[rows, :n]
            yb, sv = _fwd(c, xb, W, rev)
            if fault == "reverse_from_L" and rev and n < L and not planted:
                # the sweep of one short utterance starts at frame L - 1, over the padding frames' data
                yb = np.asarray(_fwd(c, x[rows, :L], W, rev)[0])[:, :n]
                planted = True
            if fault == "state_zeroed_at_4" and i == 0 and gi == 0:
                # the state carried into the fifth step (4 in sweep order) is zero: the sweep restarts there
                yb = np.array(yb)
                if rev:
                    yb[:, :n - 4] = np.asarray(_fwd(c, xb[:, :n - 4], W, rev)[0])
                else:
                    yb[:, 4:] = np.asarray(_fwd(c, xb[:, 4:], W, rev)[0])
            y[rows, :n] = np.asarray(yb)
            dx[rows, :n] += np.asarray(_bwd(c, xb, W, sv, dy[rows, :n, i * H:(i + 1) * H], grads, rev, scale))
            if dtype == np.float64 and fault is None:
                gates += [np.asarray(sv[k]).ravel() for k in (("z", "r") if c.cell == "gru" else ("i", "f", "o"))]
                xb64, W64, sv64 = np.asarray(xb), {k: np.asarray(v) for k, v in W.items()}, \
                    {k: np.asarray(v) for k, v in sv.items()}
                amax = max(amax, _preact_max(c, xb64, W64, sv64))
        T[f"y[{i}]"] = y
        for k in d.W[i]:
            T[f"d{k}[{i}]"] = np.asarray(grads[k])
    T["dx"] = dx
    pad = np.arange(L)[None, :] >= lens[:, None]
    if fault == "overwritten":
        T[f"d{_first_grad_key(c)}[0]"] = T[f"d{_first_grad_key(c)}[0]"] - PREFILL
    if fault == "padding_1e-30":
        b, t = np.argwhere(pad)[0]
        T["y[0]"][b, t, 0] = 1e-30
    if fault == "row16_from_15":
        T["y[0]"][16] = T["y[0]"][15]
    sat = 0.0
    if gates:
        g = np.concatenate(gates)
        sat = float(((g < 1e-6) | (g > 1 - 1e-6)).mean())
    return Ref(T, pad, sat, amax)


@functools.lru_cache(maxsize=None)
def reference(c, leg=0, dtype=np.float64, chunked=False, fault=None):
    """The oracle's gru/lstm_seq_fwd/bwd on case c in `dtype`: {name: tensor} for y per direction, dx and every
    weight / bias gradient (pre-filled with PREFILL, accumulated with SCALE), the padding mask, and for float64 the
    saturated fraction of the sigmoid gates and the largest |pre-activation|.  chunked: the float32 restatement
    with ChunkedK products.  fault: one of FAULTS planted (float64)."""
    with np.errstate(over="ignore"):
        return _reference(c, leg, dtype, chunked, fault)


# --------------------------------------------------------------------------- the checker

def check(got, ref64, ref32, name):
    """One output tensor against the float64 reference.  The bar is min(16 x the float32 restatement's own error,
    1e-4 of max|ref|): the floor is measured on the reference, never on the kernel.  Returns err / floor."""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, f"{name}: shape {got.shape}, expected {ref64.shape}"
    assert np.isfinite(got).all(), f"{name}: non-finite values"
    scale = float(np.abs(ref64).max())
    err = float(np.abs(got - ref64).max())
    if scale == 0.0:
        print(f"rnn {name}: reference is exactly 0, max|got| {err:.3e}")
        assert err <= ATOL_ZERO, f"{name}: reference is exactly 0, max |got| {err:.3e} > {ATOL_ZERO:.0e}"
        return 0.0
    floor = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    bar = min(FLOOR_FACTOR * floor, RTOL * scale)
    print(f"rnn {name}: max|got - ref| {err:.3e}, fp32 restatement {floor:.3e}, bar {bar:.3e} "
          f"(max|ref| {scale:.3e})")
    assert err <= bar, f"{name}: max|got - ref| {err:.3e} > bar {bar:.3e} (floor {floor:.3e}, max|ref| {scale:.3e})"
    return err / floor if floor > 0 else 0.0


def check_all(got, c, leg=0, tag=""):
    """Every tensor of case c (got: {name: array}, the names of reference(c).tensors) through check(), and exact
    zeros on the padding frames of y and dx.  Returns {name: err / floor}."""
    r64, r32 = reference(c, leg), reference(c, leg, np.float32)
    assert set(got) == set(r64.tensors), sorted(set(got) ^ set(r64.tensors))
    ratios = {}
    for k in r64.tensors:
        ratios[k] = check(got[k], r64.tensors[k], r32.tensors[k], f"{c.cell} {case_id(c)}{tag} {k}")
        if k == "dx" or k.startswith("y["):
            p = np.asarray(got[k])[r64.pad]
            assert (p == 0).all(), f"{case_id(c)}{tag} {k}: {int((p != 0).sum())} non-zero values on padding frames"
    return ratios
