"""Decode / validation timings on one GPU (DESIGN.md "Evaluate on the device"); not bench.py's flagship number.

  (a) equal-length beam search, config-2 decoder widths, B = 32, L = 128, K = 5: the shared-annotation path
      against an older build of the library (--parent-lib: its libs2s_hip.so, loaded beside this build's in the
      same process) and against this build's replicated arm (s2s_debug_beam_replicate);
  (b) a ragged batch, 32 utterances with L uniform in [64, 256]: one call with frame_lengths against what a caller
      of the older build had to do, 32 calls at B = 1 on each utterance's own frames;
  (c) ChorowskiBaseline.forward against the full step at config 2 (B = 32, L = 128, T = 40), graph mode: this
      build's step and, with --parent-lib, the older build's s2s_model_step on a graph-mode context of its own.

  (d) the conv + BiLSTM model's decoder (timit/timit.lua:126-145: LSTM(400, 400), A = 256, scoreDepth 150 on 160
      channels, hybrid attention kW = 5 / 16 maps, external decoder_mlp through the stepwise entry points), B = 32,
      K = 5: (i) equal lengths, share_hybrid_search on against off, with the workspace of each; (ii) mixed L', one
      ragged call against the equal-L' groups ConvBiLSTMAttentionModel._search runs by default.

Every arm is warmed up, timed with device events around the whole call (the search's own host polls included),
and the arms alternate inside one process, `--repeats` times each.  Prints one JSON object and writes it to --out.

  python tools/bench_decode.py --out profiles/decode/bench_decode.json --skip d [--parent-lib /path/to/libs2s_hip.so]
  python tools/bench_decode.py --out profiles/decode/bench_decode_hybrid.json --skip a,b,c
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "seq2seq-attention-asr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

S, A, SC, O, M, KW, EOS = 256, 512, 512, 62, 64, 7, 23


class BeamLib:
    """The few beam-search symbols both builds export, bound on a library handle of its own."""

    def __init__(self, path):
        from s2s_amd import _lib
        self.dims_t = _lib.s2s_attn_dims
        self.lib = lib = ctypes.CDLL(path)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.s2s_ctx_create.restype, lib.s2s_ctx_create.argtypes = ci, [ci, ctypes.POINTER(vp)]
        lib.s2s_last_error.restype = ctypes.c_char_p
        lib.s2s_attn_beam_workspace_bytes.restype = ctypes.c_size_t
        lib.s2s_attn_beam_workspace_bytes.argtypes = [ctypes.POINTER(self.dims_t), ci, ci]
        lib.s2s_attn_beam_search.restype = ci
        lib.s2s_attn_beam_search.argtypes = [vp, vp, ctypes.POINTER(self.dims_t), vp, vp, ci, ci, ci, vp, ci, vp, vp,
                                             vp, ctypes.c_size_t]
        self.ragged = getattr(lib, "s2s_attn_beam_search_ragged", None)
        if self.ragged is not None:
            self.ragged.restype = ci
            self.ragged.argtypes = [vp, vp, ctypes.POINTER(self.dims_t), vp, vp, ci, ci, ci, vp, vp, ci, vp, vp, vp,
                                    ctypes.c_size_t]
        self.ctx = vp()
        assert lib.s2s_ctx_create(torch.cuda.current_device(), ctypes.byref(self.ctx)) == 0

    def search(self, h, params, K, maxlen, frame_lengths=None, maxlens=None):
        """h (B, L, A) -> (tokens, lengths, scores); the workspace is allocated outside the timed region by warm-up
        calls of the same shape (torch's caching allocator)."""
        from s2s_amd.nn import stream_ptr
        B, L = h.shape[0], h.shape[1]
        d = self.dims_t(B, L, 1, A, SC, S, O, M, KW, 0.0, 0.0)
        if frame_lengths is not None:
            d.frame_lengths = frame_lengths.data_ptr()
        n = self.lib.s2s_attn_beam_workspace_bytes(ctypes.byref(d), K, maxlen)
        ws = torch.empty(n, dtype=torch.uint8, device=h.device)
        out = torch.empty((B, maxlen + 1), dtype=torch.int32, device=h.device)
        olen = torch.empty(B, dtype=torch.int32, device=h.device)
        osc = torch.empty(B, dtype=torch.float32, device=h.device)
        pa = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
        head = (self.ctx, stream_ptr(), ctypes.byref(d), h.data_ptr(), pa, EOS, K, maxlen)
        tail = (out.data_ptr(), maxlen + 1, olen.data_ptr(), osc.data_ptr(), ws.data_ptr(), n)
        rc = self.ragged(*head, maxlens.data_ptr(), *tail) if maxlens is not None else \
            self.lib.s2s_attn_beam_search(*head, *tail)
        if rc != 0:
            raise RuntimeError(self.lib.s2s_last_error().decode())
        return out, olen, osc, n


class StepLib:
    """s2s_model_step of a library handle of its own, on a graph-mode, side-stream context (the bench's timed form)."""

    def __init__(self, path, model, B, L, T):
        from s2s_amd import _lib
        self.lib = lib = ctypes.CDLL(path)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.s2s_ctx_create.restype, lib.s2s_ctx_create.argtypes = ci, [ci, ctypes.POINTER(vp)]
        lib.s2s_ctx_set_flags.restype, lib.s2s_ctx_set_flags.argtypes = ci, [vp, ci]
        lib.s2s_last_error.restype = ctypes.c_char_p
        lib.s2s_model_workspace_bytes.restype = ctypes.c_size_t
        lib.s2s_model_workspace_bytes.argtypes = [ctypes.POINTER(_lib.s2s_model_dims)]
        lib.s2s_model_step.restype = ci
        lib.s2s_model_step.argtypes = [vp, vp, ctypes.POINTER(_lib.s2s_model_dims), vp, vp, vp, vp, ctypes.c_float, ci,
                                       vp, vp, vp, ctypes.c_size_t]
        self.ctx = vp()
        assert lib.s2s_ctx_create(torch.cuda.current_device(), ctypes.byref(self.ctx)) == 0
        assert lib.s2s_ctx_set_flags(self.ctx, _lib.S2S_CTX_GRAPH | _lib.S2S_CTX_OVERLAP) == 0
        self.d = model.dims(B, L, T)
        n = lib.s2s_model_workspace_bytes(ctypes.byref(self.d))
        self.ws = torch.empty(n, dtype=torch.uint8, device=model.device)
        self.params, self.grads = model.params, torch.zeros_like(model.params)
        self.logp = torch.empty((B, T, O), dtype=torch.float32, device=model.device)
        self.nll = torch.empty(B, dtype=torch.float32, device=model.device)
        self.flags = _lib.S2S_ZERO_GRADS | _lib.S2S_NORMALIZE_NLL

    def step(self, x, y):
        from s2s_amd.nn import stream_ptr
        rc = self.lib.s2s_model_step(self.ctx, stream_ptr(), ctypes.byref(self.d), self.params.data_ptr(),
                                     self.grads.data_ptr(), x.data_ptr(), y.data_ptr(), 1.0 / x.shape[0], self.flags,
                                     self.logp.data_ptr(), self.nll.data_ptr(), self.ws.data_ptr(), self.ws.numel())
        if rc != 0:
            raise RuntimeError(self.lib.s2s_last_error().decode())
        return self.logp


def decoder_params(seed, dev):
    """The 17 decoder parameters in s2s_attn order, reset() scales, output and score weights x 3 so the searches are
    not over uniform log-probabilities."""
    g = torch.Generator().manual_seed(seed)
    shapes = [("V", (SC, A), A), ("Ws", (SC, S), S), ("bs", (SC,), S), ("we", (1, SC), SC), ("Wy", (S, O), O),
              ("by", (S,), O), ("Wc", (S, A), A), ("bc", (S,), A), ("Wd", (S, 2 * S), 2 * S), ("bd", (S,), 2 * S),
              ("Wz", (S, 2 * S), 2 * S), ("Wr", (S, 2 * S), 2 * S), ("Wh", (S, 2 * S), 2 * S),
              ("Wm", (M * KW, S + A), S + A), ("bm", (M * KW,), S + A), ("Wo", (O, M), M), ("bo", (O,), M)]
    out = []
    for name, shp, fan in shapes:
        t = (torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) / fan ** 0.5
        if name in ("Wo", "Wy", "Wm", "we"):
            t = t * 3
        out.append(t.float().to(dev).contiguous())
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def alternate(arms, repeats, warmup=2):
    """arms: name -> callable.  Returns name -> {ms: [...], median_ms, spread_ms (max - min)} and the last results."""
    last = {}
    for _ in range(warmup):
        for n, f in arms.items():
            last[n] = f()
    torch.cuda.synchronize()
    ms = {n: [] for n in arms}
    for _ in range(repeats):
        for n, f in arms.items():
            t, last[n] = timed(f)
            ms[n].append(round(t, 4))
    return {n: dict(ms=v, median_ms=round(statistics.median(v), 4), spread_ms=round(max(v) - min(v), 4))
            for n, v in ms.items()}, last


def hybrid_arm(s2s_amd, _lib, rng, repeats, B=32, K=5, L=60):
    """Arm (d): the conv + BiLSTM model's own decoder module, searched with share_hybrid_search on and off."""
    model = s2s_amd.ConvBiLSTMAttentionModel(123, 62, generator=torch.Generator().manual_seed(1)).cuda()
    att, eos = model.decoder, 61
    with torch.no_grad():  # as decoder_params: searches over log-probabilities that are not uniform
        att.own["we"].mul_(3.0)
        att.own["Wy"].mul_(3.0)
        att.own["hybU"].mul_(4.0)
        [m for m in att.decoder_mlp.modules if hasattr(m, "weight")][-1].weight.mul_(3.0)
    dev = att.own["V"].device
    h = torch.tensor(rng.standard_normal((B, L, 256)) * 1.5, dtype=torch.float32, device=dev)

    def search(on, *a, **k):
        att.share_hybrid_search = on
        try:
            return att.BeamSearch(*a, **k)
        finally:
            att.share_hybrid_search = False

    def ws_bytes(on):
        d = att._dims(h, 1)
        d.beam_share_hybrid = int(on)
        return int(_lib.lib.s2s_attn_beam_workspace_bytes(ctypes.byref(d), K, L))

    t, last = alternate({"shared": lambda: search(True, h, eos, K, L),
                         "replicated": lambda: search(False, h, eos, K, L)}, repeats)
    sh, rp = last["shared"], last["replicated"]
    same = bool(torch.equal(sh[0], rp[0]) and torch.equal(sh[1], rp[1]))
    out = {"decoder": dict(S=400, A=256, Sc=160, kW=5, maps=16, lstm=True, external_mlp=True), "B": B, "K": K,
           "i_equal_length": dict(L=L, arms=t, tokens_equal=same,
                                  scores_bitwise_equal=bool(torch.equal(sh[2], rp[2])),
                                  mean_prediction_length=float(sh[1].float().mean()),
                                  workspace_bytes={"shared": ws_bytes(True), "replicated": ws_bytes(False)})}
    # (ii) L' of 32 utterances with raw frames uniform in [120, 480] behind the front-end's three halvings
    Lp = sorted(int(x) // 8 for x in rng.integers(120, 481, B))
    limits = [8 * lp for lp in Lp]
    hm = torch.tensor(rng.standard_normal((B, max(Lp), 256)) * 1.5, dtype=torch.float32, device=dev)

    def model_search(on):
        att.share_hybrid_search, model.eval_groups = on, []
        try:
            return model._search(hm, Lp, limits, eos, K)
        finally:
            att.share_hybrid_search = False

    t, last = alternate({"ragged_one_call": lambda: model_search(True), "equal_Lp_groups": lambda: model_search(False)},
                        repeats, warmup=1)
    rg, gr = last["ragged_one_call"], last["equal_Lp_groups"]
    same = sum(int(rg[1][i]) == int(gr[1][i]) and torch.equal(rg[0][i, :int(rg[1][i])], gr[0][i, :int(gr[1][i])])
               for i in range(B))
    out["ii_mixed_lengths"] = dict(Lp=Lp, groups=len(set(Lp)), arms=t, identical_predictions=same,
                                   mean_prediction_length=float(rg[1].float().mean()),
                                   ratio_groups_over_ragged=round(
                                       t["equal_Lp_groups"]["median_ms"] / t["ragged_one_call"]["median_ms"], 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libs2s_hip.so of the build to compare against")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip", default="", help="comma list of a,b,c,d")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode needs a GPU"
    import s2s_amd
    from s2s_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    new = BeamLib(_lib.LIB_PATH)
    old = BeamLib(args.parent_lib) if args.parent_lib else None
    knob = new.lib.s2s_debug_beam_replicate
    knob.argtypes, knob.restype = [ctypes.c_int], None
    params = decoder_params(11, dev)
    rng = np.random.default_rng(11)
    res = {"device": torch.cuda.get_device_name(dev), "repeats": args.repeats, "parent_lib": bool(old),
           "widths": dict(S=S, A=A, Sc=SC, O=O, M=M, window=KW)}
    skip = set(args.skip.split(","))

    def replicated(*a, **k):
        knob(1)
        try:
            return new.search(*a, **k)
        finally:
            knob(0)

    if "a" not in skip:
        B, L, K = 32, 128, 5
        h = torch.tensor(rng.standard_normal((B, L, A)) * 1.5, dtype=torch.float32, device=dev)
        arms = {"shared": lambda: new.search(h, params, K, L), "replicated_arm": lambda: replicated(h, params, K, L)}
        if old:
            arms["parent"] = lambda: old.search(h, params, K, L)
        t, last = alternate(arms, args.repeats)
        ref = last["parent" if old else "replicated_arm"]
        same = bool(torch.equal(last["shared"][0], ref[0]) and torch.equal(last["shared"][1], ref[1]))
        res["a_equal_length"] = dict(B=B, L=L, K=K, arms=t, tokens_equal=same,
                                     scores_bitwise_equal=bool(torch.equal(last["shared"][2], ref[2])),
                                     mean_prediction_length=float(last["shared"][1].float().mean()),
                                     workspace_bytes={n: int(r[3]) for n, r in last.items()})
    if "b" not in skip:
        N, K = 32, 5
        lens = sorted(int(x) for x in rng.integers(64, 257, N))
        L = max(lens)
        h = torch.tensor(rng.standard_normal((N, L, A)) * 1.5, dtype=torch.float32, device=dev)
        fl = torch.tensor(lens, dtype=torch.int32, device=dev)
        own = [h[i, :lens[i]].contiguous()[None] for i in range(N)]
        one = old or new

        def per_utterance():
            return [(replicated if one is new else one.search)(own[i], params, K, lens[i]) for i in range(N)]

        arms = {"ragged_one_call": lambda: new.search(h, params, K, L, frame_lengths=fl, maxlens=fl),
                "per_utterance_32_calls": per_utterance}
        t, last = alternate(arms, args.repeats, warmup=1)
        rag, per = last["ragged_one_call"], last["per_utterance_32_calls"]
        same = sum(int(rag[1][i]) == int(per[i][1][0]) and
                   torch.equal(rag[0][i, :int(rag[1][i])], per[i][0][0, :int(per[i][1][0])]) for i in range(N))
        res["b_ragged"] = dict(N=N, K=K, lengths=lens, arms=t, identical_predictions=same,
                               per_utterance_arm="parent build" if old else "this build, replicated arm",
                               ratio_per_utterance_over_ragged=round(
                                   t["per_utterance_32_calls"]["median_ms"] / t["ragged_one_call"]["median_ms"], 3))
    if "c" not in skip:
        B, L, T = 32, 128, 40
        model = s2s_amd.ChorowskiBaseline(s2s_amd.ModelConfig(), seed=4321, graph=True, overlap=True)
        x = torch.tensor(rng.standard_normal((B, L, 123)), dtype=torch.float32, device=dev)
        y = torch.tensor(rng.integers(0, O, (B, T)), dtype=torch.int32, device=dev)
        arms = {"forward_only": lambda: model.forward(x, y), "full_step": lambda: model.step(x, y)}
        if args.parent_lib:
            parent = StepLib(args.parent_lib, model, B, L, T)
            arms["parent_full_step"] = lambda: parent.step(x, y)
        # on a stream of its own: a graph-mode context captures and replays only on a non-default stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            t, last = alternate(arms, max(args.repeats, 10), warmup=3)
        torch.cuda.synchronize()
        cap, rep = ctypes.c_long(), ctypes.c_long()
        _lib.lib.s2s_ctx_graph_stats(model.ctx.handle, ctypes.byref(cap), ctypes.byref(rep), None)
        res["c_forward_only"] = dict(B=B, L=L, T=T, mode="hipGraph replay, side-stream layout", arms=t,
                                     graphs_captured=cap.value, graph_replays=rep.value)
        if args.parent_lib:  # the same step: the older build's logp equals this build's full step's bit for bit
            res["c_forward_only"]["parent_logp_bitwise_equal"] = bool(torch.equal(last["parent_full_step"],
                                                                                   last["full_step"][1]))
    if "d" not in skip:
        res["d_hybrid_conv_decoder"] = hybrid_arm(s2s_amd, _lib, rng, args.repeats)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
