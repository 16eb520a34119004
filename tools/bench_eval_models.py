"""Time Evaluate and one step_ragged epoch slice of the conv + BiLSTM and VGG models on mixed-length data.

64 synthetic utterances with TIMIT-like lengths (frames uniform in [120, 480], labels in [15, 50]) at each model's
reference widths.  Two arms per measurement, alternating in one process, medians of --reps, device events around
the whole call:

  ragged    model.Evaluate(packed, K, max_batch) / model.step_ragged(packed, max_batch): padded, length-masked
            batches assembled on the device (s2s_amd.data.PackedUtterances)
  loop      the reference trainer's shape, one utterance at a time, through interfaces that predate the ragged
            surface: model.step(x[None], y[None]) per utterance for training; encoder.forward + decoder.forward +
            nll_seed + decoder.BeamSearch(h, eos, K, limit) per utterance for validation

For the conv + BiLSTM model a third measurement times Evaluate with decoder.share_hybrid_search on (one ragged
search per padded batch) against off (one search per equal-L' group), and reports whether the two agree.

No threshold is attached to these numbers; they are written down (--out, default
profiles/models_ragged/bench.json) so that the next change can be measured against them.

    python tools/bench_eval_models.py [--models conv,vgg] [--n 64] [--reps 5] [--max-batch 32] [--K 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "seq2seq-attention-asr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def corpus(kind, n, F, O, seed):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    eos = O - 1
    xs, ys = [], []
    for _ in range(n):
        L, T = int(rng.integers(120, 481)), int(rng.integers(15, 51))
        shape = (L, F) if kind == "conv" else (3, L, F)
        xs.append(torch.tensor(rng.standard_normal(shape).astype(np.float32), device="cuda"))
        y = rng.integers(0, eos, T)
        y[-1] = eos
        ys.append(torch.tensor(y.astype(np.int32), device="cuda"))
    return xs, ys, eos


def bench_model(kind, args):
    import torch

    import s2s_amd
    from s2s_amd.data import PackedUtterances
    from s2s_amd.nn import nll_seed
    g = torch.Generator().manual_seed(1)
    if kind == "conv":
        model = s2s_amd.ConvBiLSTMAttentionModel(123, 62, generator=g).cuda()  # timit/timit.lua:106-145
        F, O, axis = 123, 62, 0
    else:
        model = s2s_amd.VGGAttentionModel(40, outputDepth=29, generator=g).cuda()  # librispeech/model_vgg.lua
        F, O, axis = 40, 29, 1
    xs, ys, eos = corpus(kind, args.n, F, O, 7)
    pk = PackedUtterances(xs, ys)
    N, factor = len(xs), model.maxlen_factor

    def train_ragged():
        model.step_ragged(pk, None, max_batch=args.max_batch)

    def train_loop():
        model.zeroGradParameters()
        for x, y in zip(xs, ys):
            model.step(x[None], y[None], 1.0 / N)

    def eval_ragged():
        model.Evaluate(pk, None, K=args.K, max_batch=args.max_batch)

    def eval_loop():
        for x, y in zip(xs, ys):
            h = model.encoder.forward(x[None])
            logp = model.decoder.forward([h, y[None]])
            nll_seed(logp, y[None])
            model.decoder.BeamSearch(h[0], eos, args.K, factor * x.shape[axis])

    def eval_shared():
        model.decoder.share_hybrid_search = True
        try:
            return model.Evaluate(pk, None, K=args.K, max_batch=args.max_batch)
        finally:
            model.decoder.share_hybrid_search = False

    def eval_grouped():
        return model.Evaluate(pk, None, K=args.K, max_batch=args.max_batch)

    out = {"model": kind, "utterances": N, "frames": [int(x.shape[axis]) for x in xs],
           "labels": [int(y.numel()) for y in ys], "K": args.K, "max_batch": args.max_batch, "reps": args.reps}
    measurements = [("step_ragged_epoch_slice", (("ragged", train_ragged), ("loop", train_loop))),
                    ("evaluate", (("ragged", eval_ragged), ("loop", eval_loop)))]
    if kind == "conv":
        measurements.append(("evaluate_share_hybrid_search", (("shared", eval_shared), ("grouped", eval_grouped))))
        sh, gr = eval_shared(), eval_grouped()
        out["evaluate_share_hybrid_search_agreement"] = {
            "identical_predictions": sum(a.tolist() == b.tolist() for a, b in zip(sh[3], gr[3])),
            "per_shared": sh[2], "per_grouped": gr[2]}
    if args.only:
        measurements = [m for m in measurements if m[0] in args.only.split(",")]
    for name, arms in measurements:
        for _, fn in arms:
            fn()  # warm-up: lazily grown buffers, first-launch costs
        ms = {a: [] for a, _ in arms}
        for _ in range(args.reps):
            for a, fn in arms:
                ms[a].append(timed(fn))
        out[name] = {a: {"median_ms": statistics.median(v), "all_ms": v} for a, v in ms.items()}
        (new, _), (base, _) = arms
        out[name][f"speedup_{base}_over_{new}"] = out[name][base]["median_ms"] / out[name][new]["median_ms"]
        print(name, kind, {a: round(out[name][a]["median_ms"], 1) for a in ms}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="conv,vgg")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--only", default="", help="comma list of measurements to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "models_ragged", "bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_eval_models.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "results": [bench_model(k, args) for k in args.models.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
