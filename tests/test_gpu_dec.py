"""GPU: the attention decoder (csrc/attn.hip with dec_steps.inc, attn_persist.inc, dec_xcd.inc, dec_xcd_lstm.inc) on
every route -- the per-step launches with and without the fold, the persistent kernels, the XCD-local kernels
resident and streamed, the XCD-local LSTM kernels with the fused Maxout head -- with hybrid filters of 1, 4, 5 and 8
taps, dropout, ragged lengths, and data whose attention is sharp and moves across chunk edges.  Every output tensor
is held to the float64 oracle at a bar taken from the oracle's own float32 error (tests/dec_case.py: min(16 x floor,
1e-4 max|ref|); tests/test_dec_case_cpu.py shows, without a GPU, that the cases are what this file takes them for and
that the checker rejects planted faults).  Each case runs four launches on the same module -- its shape; other data,
halved weights, a shorter L and a longer T; a shorter T; the first again, bitwise -- with gradients accumulated
onto a prefill, on poisoned buffers, and asserts the route the library recorded."""
import numpy as np
import pytest
import torch

import dec_case as dc
import paths
from test_gpu_parity import _clean_status, _poisoned_buffers

pytestmark = pytest.mark.gpu

MODES = {"auto": paths.MODE_AUTO, "step": paths.MODE_STEP, "persist": paths.MODE_PERSIST}
assert (paths.STEPS, paths.PERSIST, paths.XCD, paths.XCD_LSTM) == (dc.STEPS, dc.PERSIST, dc.XCD, dc.XCD_LSTM)


@pytest.fixture(scope="module")
def s2s():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import s2s_amd
    return s2s_amd


def cu(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _module(s2s, c):
    """nn.Attention(GRU | LSTM, MaxoutMLP) with the case's parameters of leg 0; returns it and a function giving
    {oracle name: (weight, gradient)} (looked up at every use: the score-channel padding rebinds storage)."""
    P = dc.build(c).P
    cell = s2s.GRU(c.S, c.S) if c.cell == "gru" else s2s.LSTM(c.S, c.S, peepholes=False)
    mlp = s2s.MaxoutMLP(c.S + c.A, c.M, c.K, c.O, dropout=c.dropout)
    att = s2s.Attention(cell, mlp, c.Sc, c.kW if c.nF else 10, c.nF, c.S, c.A, c.O, True, c.pen)

    def look():
        t = {n: (att.own[n], att.own_grad[n]) for n in dc.param_names(c) if n in att.own}
        if c.cell == "gru":
            t.update(zip(("dec.Wz", "dec.Wr", "dec.Wh"), zip(cell.weight, cell.gradWeight)))
        else:
            g = cell.named(grads=True)
            t.update({"dec." + n: (w, g[n]) for n, w in cell.named().items()})
        t.update(zip(("Wm", "bm", "Wo", "bo"), zip(mlp.weight, mlp.gradWeight)))
        return t
    tens = look()
    assert sorted(tens) == sorted(P), sorted(set(tens) ^ set(P))
    with torch.no_grad():
        for n, (w, _) in tens.items():
            assert tuple(w.shape) == P[n].shape, (n, tuple(w.shape), P[n].shape)
            w.copy_(torch.tensor(P[n]))
    return att.cuda(), look


def _launch(att, look, c, leg):
    """Forward, then backward with SCALE onto gradients pre-filled with PREFILL, on the leg's data; returns the
    tensors under the reference's names, the Maxout winners and indicators, and the recorded decisions."""
    d = dc.build(c, leg)
    att.frame_lengths, att.label_lengths = d.flen, d.tlen
    att.dropout_mask = None if d.mask is None else cu(d.mask)
    hs, labels, dlogp = cu(d.h), cu(d.labels, torch.int32), cu(d.dlogp)
    with paths.decisions() as dec:
        logp = att.forward([hs, labels]).cpu().numpy()
        got = {"logp": logp, "alpha": att.alpha().cpu().numpy(), "mono_ind": att.mono_ind().cpu().numpy(),
               "maxout_argmax": att.maxout_argmax().cpu().numpy()}
        if d.mask is not None:
            used = att.dropout_mask_used().cpu().numpy()
            assert np.array_equal(used, d.mask), "the injected mask was not the one used"
        with torch.no_grad():
            for _, g in look().values():
                g.fill_(dc.PREFILL)
        got["dh"] = att.backward([hs, None], dlogp, dc.SCALE)[0].cpu().numpy()
        torch.cuda.synchronize()
    for n, (_, g) in look().items():
        got["d" + n] = g.cpu().numpy()
    return got, dec


def _took_route(dec, c, leg):
    """The recorded route of a leg against the table (leg 0 and its repeat) or the dispatch rules restated in
    dec_case.route (the other legs' shapes)."""
    L, T = dc.leg_shape(c, leg)
    path, plan, _ = (c.path, c.plan, c.fold) if leg in (0, 3) else dc.route(c, L, T)
    for name in ("dec.fwd.path", "dec.bwd.path"):
        assert dec.count(name) == 1, f"{name} recorded {dec.count(name)} times"
        paths.took(dec, name, path)
    if path in (dc.XCD, dc.XCD_LSTM):
        got = tuple(dec[n] for n in ("dec.U", "dec.nchains", "dec.XLC", "dec.NCH", "dec.res"))
        assert got == plan, (got, plan)
        paths.took(dec, "dec.r4", int(path == dc.XCD_LSTM or plan[0] <= 4))
    if path == dc.PERSIST:
        assert dec.count("dec.persist_res") == 2
        if c.persist_res is not None and leg != 1:
            paths.took(dec, "dec.persist_res", c.persist_res)
    return f"path {dec['dec.fwd.path']} plan {plan} persist_res {dec.get('dec.persist_res')} r4 {dec.get('dec.r4')}"


@pytest.mark.parametrize("c", dc.CASES, ids=[dc.case_id(c) for c in dc.CASES])
def test_decoder_case(s2s, monkeypatch, c):
    """One case of tests/dec_case.py: legs 0 to 3 on the same module, each with the recorded route asserted and
    every tensor through the checker; leg 3 equals leg 0 bitwise (the decoder has no float atomics); the context's
    status is clean at the end."""
    _poisoned_buffers(monkeypatch, s2s)
    if c.stream is None:
        monkeypatch.delenv("S2S_DEC_STREAM", raising=False)
    else:
        monkeypatch.setenv("S2S_DEC_STREAM", c.stream)
    att, look = _module(s2s, c)
    fails, first = [], None
    try:
        with paths.dec_mode(MODES[c.mode]):
            for leg in range(dc.NLEGS):
                if leg in (1, 2):  # leg 1 halves every weight in place, leg 2 restores them (exact in binary)
                    with torch.no_grad():
                        for w, _ in look().values():
                            w.mul_(0.5 if leg == 1 else 2.0)
                got, dec = _launch(att, look, c, leg)
                rec = _took_route(dec, c, leg)
                ratios, f = dc.check_all(got, c, leg)
                fails += f
                worst = max(ratios, key=ratios.get)
                print(f"dec {dc.case_id(c)} leg {leg}: {rec}; largest err / floor {ratios[worst]:.2f} ({worst})")
                if leg == 0:
                    first = got
                if leg == 3:
                    r = dc.reference(c, 0)
                    for k, v in got.items():
                        a, b = np.array(v), np.array(first[k])
                        if k in ("logp", "alpha", "mono_ind", "maxout_argmax"):  # (padding steps: not specified)
                            a[r.tpad], b[r.tpad] = 0, 0
                        if not np.array_equal(a, b):
                            fails.append(f"{dc.case_id(c)} {k}: leg 3 differs from leg 0, max |d| "
                                         f"{np.abs(a.astype(np.float64) - b).max():.3e}")
    finally:
        _clean_status(s2s)
    assert not fails, "\n".join(fails)
