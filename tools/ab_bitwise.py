"""Bitwise A/B of the decoder paths between two builds: run once per library (S2S_HIP_LIB), then compare.
  S2S_HIP_LIB=.../ab/base.so python tools/ab_bitwise.py save ab_out/ab_base.pt
  S2S_HIP_LIB=.../ab/new.so  python tools/ab_bitwise.py save ab_out/ab_new.pt
  python tools/ab_bitwise.py cmp ab_out/ab_base.pt ab_out/ab_new.pt
Arms (`save PATH ARM` runs one of them alone, e.g. under a kernel trace):
  conv         one conv + BiLSTM model step (timit/timit.lua:106-145: LSTM encoder, LSTM decoder, hybrid attention:
               the xcd_lstm path) and a hybrid beam search
  gru0/1/2     one GRU-decoder model step at the small XCD widths (S=64, A=128, Sc=128) under s2s_debug_dec_mode
               0 (auto: the xcd path), 1 (per-step launches), 2 (the persistent kernels)
  gru_hybrid   a GRU decoder with hybrid attention, forward and backward: the folded per-step path
  beam         a content-attention beam search (the shared-annotation path)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seq2seq-attention-asr_amd"))

S, A, SC, O, M, KWIN = 64, 128, 128, 62, 64, 7
B, L, T = 8, 48, 6


def conv(s2s_amd):
    g = torch.Generator().manual_seed(3)
    B, L, T = 8, 128, 12
    x = torch.randn((B, L, 123), generator=g).cuda()
    labels = torch.randint(0, 61, (B, T), generator=g).to(torch.int32).cuda()
    m = s2s_amd.ConvBiLSTMAttentionModel(generator=torch.Generator().manual_seed(1), penalty=0.1).cuda()
    m.zeroGradParameters()
    nll, logp = m.step(x, labels)
    out = {"nll": nll, "logp": logp, "grads": [t.clone() for t in m.parameters()[1]]}
    h = m.encoder.forward(x)
    toks, lens, scores = m.decoder.BeamSearch(h, 1, K=3, maxseqlength=6)
    out.update(beam_toks=toks, beam_scores=scores)
    return out


def gru(s2s_amd, mode):
    from s2s_amd._lib import lib
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, L, 40), generator=g).cuda()
    labels = torch.randint(0, O - 1, (B, T), generator=g).to(torch.int32).cuda()
    cfg = s2s_amd.ModelConfig(inputFrameSize=40, hiddenFrameSize=64, outputFrameSize=A // 2, scoreDepth=SC,
                              stateDepth=S, outputDepth=O, mlpDepth=M, maxoutWindow=KWIN, penalty=0.1)
    m = s2s_amd.ChorowskiBaseline(cfg, seed=2)
    lib.s2s_debug_dec_mode(mode)
    try:
        nll, logp = m.step(x, labels)
        return {"nll": nll.clone(), "logp": logp.clone(), "grads": m.grads.clone()}
    finally:
        lib.s2s_debug_dec_mode(-1)


def attention(s2s_amd, hybrid):
    gen = torch.Generator().manual_seed(7)
    att = s2s_amd.Attention(s2s_amd.GRU(S, S, generator=gen), s2s_amd.MaxoutMLP(S + A, M, KWIN, O, generator=gen), SC,
                            5 if hybrid else None, 8 if hybrid else 0, S, A, O, True, 0.1, generator=gen).cuda()
    h = torch.randn((B, L, A), generator=gen).cuda()
    return att, h, gen


def gru_hybrid(s2s_amd):
    att, h, gen = attention(s2s_amd, True)
    labels = torch.randint(0, O - 1, (B, T), generator=gen).to(torch.int32).cuda()
    dlogp = torch.randn((B, T, O), generator=gen).cuda()
    logp = att.forward([h, labels]).clone()
    att.zeroGradParameters()
    dh = att.backward([h, None], dlogp)[0].clone()
    return {"logp": logp, "dh": dh, "grads": [t.clone() for t in att.parameters()[1]]}


def beam(s2s_amd):
    att, h, _ = attention(s2s_amd, False)
    toks, lens, scores = att.BeamSearch(h, 1, K=3, maxseqlength=6)
    return {"toks": toks, "lens": lens, "scores": scores}


ARMS = {"conv": conv, "gru0": lambda s: gru(s, 0), "gru1": lambda s: gru(s, 1), "gru2": lambda s: gru(s, 2),
        "gru_hybrid": gru_hybrid, "beam": beam}


def save(path, arms):
    import s2s_amd
    out = {}
    for arm in arms:
        for k, v in ARMS[arm](s2s_amd).items():
            out[f"{arm}.{k}"] = v.cpu() if torch.is_tensor(v) else [t.cpu() for t in v]
    torch.cuda.synchronize()
    torch.save(out, path)
    print("saved", path, "arms:", " ".join(arms))


def cmp(a, b):
    A, Bd = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    assert A.keys() == Bd.keys(), "the two files hold different arms"
    for arm in sorted({k.split(".")[0] for k in A}):
        bad = []
        for k in (k for k in A if k.split(".")[0] == arm):
            if isinstance(A[k], list):
                bad += [f"{k}[{i}]" for i, (x, y) in enumerate(zip(A[k], Bd[k])) if not torch.equal(x, y)]
            elif not torch.equal(A[k], Bd[k]):
                bad.append(k)
        print(f"{arm}: bitwise equal" if not bad else f"{arm}: DIFFER: {bad}")


if __name__ == "__main__":
    save(sys.argv[2], sys.argv[3:] or list(ARMS)) if sys.argv[1] == "save" else cmp(sys.argv[2], sys.argv[3])
