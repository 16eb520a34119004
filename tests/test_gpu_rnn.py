"""GPU: the GRU and LSTM layers (csrc/gru.hip, gru_persist.hip, lstm.hip, lstm_persist.hip) at every persistent
width, both chain rounds and the first shapes past them, short and ragged sequences, saturated gates, and a
relaunch of the same module on other data -- every output tensor against the float64 oracle, at a bar taken from
the oracle's own float32 error (tests/rnn_case.py: min(16 x floor, 1e-4 max|ref|); tests/test_rnn_case_cpu.py
shows, without a GPU, that the floor is usable, that another float32 order keeps a factor 4 from the bar, and that
the checker rejects planted faults).  Each case also asserts the kernel path the library recorded."""
import numpy as np
import pytest
import torch

import paths
import rnn_case as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def s2s():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import s2s_amd
    return s2s_amd


def cu(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def _names(c):
    if c.cell == "gru":
        return ["Wz", "Wr", "Wh"]
    return [f"{p}{q}{s}" for q in rc.LSTM_GATES for p, s in (("W", "x"), ("b", "x"), ("W", "h"), ("b", "h"))] + \
        ([f"{p}{q}c" for q in ("i", "f", "o") for p in ("W", "b")] if c.peep else [])


def _module(s2s, c):
    d = rc.build(c)
    cells = []
    for W in d.W:
        cell = s2s.GRU(c.D, c.H) if c.cell == "gru" else s2s.LSTM(c.D, c.H, peepholes=c.peep)
        if c.cell == "lstm":
            assert cell.names == _names(c)
        for w, k in zip(cell.weight, _names(c)):  # the case's own draw of the module's initialisation
            assert tuple(w.shape) == W[k].shape
            w.copy_(torch.from_numpy(W[k]))
        cells.append(cell)
    mod = s2s.BiRNN(*cells) if c.dirn == "bi" else s2s.RNN(cells[0], reverse=(c.dirn == "rev"))
    return mod.cuda(), cells


def _launch(mod, cells, c, leg):
    """Forward then backward on the case's data of this leg, gradients accumulated onto the prefill; returns the
    tensors under the reference's names and the recorded decisions."""
    d = rc.build(c, leg)
    mod.lengths = None if d.lens is None else d.lens
    for cell in cells:
        for g in cell.gradWeight:
            g.fill_(rc.PREFILL)
    xs, dys = cu(d.x), cu(d.dy)
    with paths.decisions() as dec:
        y = mod.forward(xs).cpu().numpy()
        dx = mod.backward(xs, dys, rc.SCALE).cpu().numpy()
        torch.cuda.synchronize()
    got = {"dx": dx}
    for i, cell in enumerate(cells):
        got[f"y[{i}]"] = y[:, :, i * c.H:(i + 1) * c.H]
        for k, g in zip(_names(c), cell.gradWeight):
            got[f"d{k}[{i}]"] = g.cpu().numpy()
    return got, dec


def _took(dec, c, path):
    if c.cell == "gru":
        paths.took(dec, "gru.fwd.path", path)
        paths.took(dec, "gru.bwd.path", path)
        paths.took(dec, "gru.fused_xproj", c.fused if path else 0)
        return f"gru.fwd.path {dec['gru.fwd.path']} gru.bwd.path {dec['gru.bwd.path']} gru.fused_xproj " \
               f"{dec['gru.fused_xproj']} gru.local {dec.get('gru.local')} gru.ring {dec.get('gru.ring')}"
    paths.took(dec, "lstm.fwd.path", path)
    paths.took(dec, "lstm.bwd.path", path)
    return f"lstm.fwd.path {dec['lstm.fwd.path']} lstm.bwd.path {dec['lstm.bwd.path']}"


def _run_case(s2s, monkeypatch, c):
    mode = "S2S_GRU_MODE" if c.cell == "gru" else "S2S_LSTM_MODE"
    monkeypatch.delenv(mode, raising=False)
    mod, cells = _module(s2s, c)
    got, dec = _launch(mod, cells, c, 0)
    rec = _took(dec, c, c.path)
    ratios = rc.check_all(got, c, 0)
    worst = max(ratios, key=ratios.get)
    print(f"rnn {c.cell} {rc.case_id(c)}: {rec}; largest err / floor {ratios[worst]:.2f} ({worst})")
    # the same module again on other x, dy and lengths with its weights halved in place: a sentinel, granule or
    # weight pack left over from the first launch would now belong to other data
    for cell in cells:
        for w in cell.weight:
            w.mul_(0.5)
    got, dec1 = _launch(mod, cells, c, 1)
    _took(dec1, c, c.path)
    ratios = rc.check_all(got, c, 1, " relaunch")
    worst = max(ratios, key=ratios.get)
    print(f"rnn {c.cell} {rc.case_id(c)} relaunch: largest err / floor {ratios[worst]:.2f} ({worst})")
    if c.ab:  # the per-step launches at the same shape, on a fresh module: the other arm meets the same bar
        monkeypatch.setenv(mode, "step")
        mod, cells = _module(s2s, c)
        got, dec_s = _launch(mod, cells, c, 0)
        _took(dec_s, c, 0)
        paths.differ(dec, dec_s, f"{c.cell}.fwd.path")
        paths.differ(dec, dec_s, f"{c.cell}.bwd.path")
        ratios = rc.check_all(got, c, 0, " step")
        worst = max(ratios, key=ratios.get)
        print(f"rnn {c.cell} {rc.case_id(c)} step: largest err / floor {ratios[worst]:.2f} ({worst})")


@pytest.mark.parametrize("c", rc.GRU_CASES, ids=[rc.case_id(c) for c in rc.GRU_CASES])
def test_gru_layer_case(s2s, monkeypatch, c):
    """nn.RNN / BiRNN over nn.GRU: y per direction, dx and the three weight gradients of each direction against
    the float64 oracle (per utterance on its unpadded slice where there are lengths), exact zeros on padding
    frames, the recorded path and x-projection form, then a relaunch on other data and, for one case of each
    persistent width, the per-step arm."""
    _run_case(s2s, monkeypatch, c)


@pytest.mark.parametrize("c", rc.LSTM_CASES, ids=[rc.case_id(c) for c in rc.LSTM_CASES])
def test_lstm_layer_case(s2s, monkeypatch, c):
    """nn.RNN / BiRNN over nn.LSTM, with and without peepholes: y per direction, dx and every weight / bias
    gradient against the float64 oracle, as test_gru_layer_case.  H = 192 without peepholes must take the per-step
    launches: the persistent kernels are instantiated for H in {64, 128, 256} only."""
    _run_case(s2s, monkeypatch, c)
