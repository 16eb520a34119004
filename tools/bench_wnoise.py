"""Weight-noise kernels (csrc/wnoise.hip) on one MI355X at the Chorowski flat layout's n = 4,356,222:
microseconds per call and achieved GB/s for sample(), backward() and mode() of AdaptiveWeightNoise /
WeightNoise, and for the Adadelta step on weight (2n).  The yardstick is the Adadelta step on n in the same
invocation (32 B per parameter: x, g, v, u read and written).

Every call is timed as a captured graph of CALLS back-to-back calls, replayed (device time without the host's
launch cost, the form a training loop replays); REPEATS windows, the median is reported, min and max beside it.
Bytes are the algorithm's: what each pass has to read and write, from the configuration (wd = weight decay on
adds the sampled parameters to both backward passes; the KL term adds mu and s to the reduction).
One JSON line per row.
Usage (GPU box): python tools/bench_wnoise.py [--calls 20] [--replays 50] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "seq2seq-attention-asr_amd")]

import torch  # noqa: E402

N_CHOROWSKI = 4_356_222


def time_graph(fn, calls, replays, repeats):
    """Median / min / max microseconds per fn() over `repeats` windows of `replays` replays of a graph of
    `calls` calls."""
    fn()
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        for _ in range(calls):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / (replays * calls))
    return statistics.median(us), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=N_CHOROWSKI)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_wnoise needs a GPU")
    from s2s_amd import optim

    n = a.n
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(1)
    g0 = torch.randn(n, device=dev, generator=gen) * 1e-3
    nll = torch.rand(32, device=dev, generator=gen) + 1.0
    rows = []

    def row(name, bytes_per_param, fn, elems=n):
        med, lo, hi = time_graph(fn, a.calls, a.replays, a.repeats)
        r = {"call": name, "n": elems, "bytes_per_param": bytes_per_param, "us": round(med, 2),
             "us_min": round(lo, 2), "us_max": round(hi, 2),
             "GBps": round(bytes_per_param * elems / med * 1e-3, 1)}
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    def flat():
        p = torch.randn(n, device=dev, generator=gen) * 0.08
        return p, g0.clone()

    # the yardstick: Adadelta on n
    p, g = flat()
    opt = optim.Adadelta(params=p, grads=g)
    yard = row("adadelta_n", 32, opt.step)

    trainer = dict(maxnorm=1.0, weightDecay=1e-4, gradnoise_eta=0.0)
    for wd in (0.0, 1e-4):
        p, g = flat()
        awn = optim.AdaptiveWeightNoise(params=p, grads=g, adalambda=1 / 32, sigma_init=0.075,
                                        **dict(trainer, weightDecay=wd))
        if wd == 0.0:
            row("awn_sample", 12, awn.sample)
            row("awn_mode", 8, awn.mode)
        awn.sample()
        extra = 4 if wd else 0
        # reduction: g, mu, s (+ p); elementwise: g, mu, s (+ p) read, g, gradmu, grads written
        row(f"awn_backward_wd{int(bool(wd))}", (12 + extra) + (12 + extra) + 12, lambda: awn.backward(nll))
        if wd:
            opt2 = optim.Adadelta(params=awn.weight, grads=awn.gradWeight)
            row("adadelta_2n", 32, opt2.step, elems=2 * n)
    p, g = flat()
    wn = optim.WeightNoise(params=p, grads=g, sigma=0.075, **trainer)
    row("wn_sample", 8, wn.sample)
    # reduction: g, p; elementwise: g, p read, g, gradWeight written
    row("wn_backward_wd1", 8 + 8 + 8, lambda: wn.backward(nll))
    p, g = flat()
    noisy = optim.AdaptiveWeightNoise(params=p, grads=g, adalambda=1 / 32, sigma_init=0.075, maxnorm=1.0,
                                      weightDecay=1e-4, gradnoise_eta=1e-3)
    noisy.sample()
    row("awn_backward_wd1_gradnoise", 44, lambda: noisy.backward(nll))
    print(json.dumps({"yardstick": "adadelta_n", "GBps": yard["GBps"],
                      "share_of_yardstick": {r["call"]: round(r["GBps"] / yard["GBps"], 3) for r in rows}}))


if __name__ == "__main__":
    main()
