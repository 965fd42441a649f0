"""Evaluation on a whole network: Nnet.ComputeProb (nnet-compute-prob: the
objective and the frame accuracy, forward only) at 4096 frames a call, on the
fused path (a last Softmax is not run: one kernel takes the sums from its
input) and on the literal path (Propagate, then one pass over the stored
output), beside a plain Propagate of the same network on the same input.

The network is a config (default tests/golden/nnet.config; --config
tests/golden/train_conv.config for the training recipes' topology).  When it
has Dropout the test model is evaluated, as the recipes do: Nnet.Copy with
the scales of tests/golden/dropout_scale.config and the Dropout layers
removed.

The three are timed in turn, call by call (each call ends in a device
synchronise), so that they see the same machine; each is reported as the
median over --steps calls with its minimum, maximum and 10th / 90th
percentiles.  `back_to_back` times them as an evaluation loop runs them:
--steps calls enqueued one after the other and one synchronise, seven rounds
in turn.  `kernel_scope_ms` is the hipEvent scope of the Softmax and of the
two ComputeProb kernels in each of the three.  Prints one JSON line.

  python scripts/compute_prob_bench.py --steps 30 --warmup 5
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))


def time_in_turn(calls, steps, warmup, sync):
    """calls: {name: function}.  Runs them round-robin, `warmup` untimed rounds
    then `steps` timed ones, each call between two sync()s; returns {name: ms
    per call, one per round}."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    sync()
    ms = {name: [] for name in calls}
    for _ in range(steps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def time_back_to_back(calls, steps, rounds, sync):
    """`steps` calls enqueued one after the other and one sync(), `rounds`
    times in turn; returns {name: ms per call of each round}."""
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            sync()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    return ms


def kernel_scopes(kcnn, calls, steps, keys):
    """hipEvent scope time per call (launch gaps included) of the profile
    entries `keys` over `steps` calls of each function."""
    out = {}
    kcnn.set_profiling(True)
    try:
        for name, fn in calls.items():
            kcnn.reset_profile()
            for _ in range(steps):
                fn()
            for line in kcnn.profile_string().strip().splitlines():
                parts = line.split("\t")
                if len(parts) >= 3 and parts[0] in keys:
                    out.setdefault(name, {})[parts[0]] = round(
                        float(parts[1].split()[0]) / int(parts[2].split()[0]), 4)
    finally:
        kcnn.set_profiling(False)
        kcnn.reset_profile()
    return out


def summary(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4), "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4)}


def random_input(net, frames, seed=20261019):
    import torch
    context = sum(c._span() for c in net.components)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randn(((context + 1) * frames, net.components[0].InputDim()), generator=gen,
                       device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--config", default=os.path.join(ROOT, "tests", "golden", "nnet.config"))
    ap.add_argument("--scales", default=os.path.join(ROOT, "tests", "golden",
                                                     "dropout_scale.config"))
    args = ap.parse_args()

    import torch
    import kcnn

    kcnn.init(0)
    kcnn.set_randn_seed(20261019)
    net = kcnn.Nnet(open(args.config).read())
    model = "as configured"
    if any(c.Type() == "DropoutComponent" for c in net.components):
        scales = [float(s) for s in open(args.scales).read().strip().split(":")]
        num_updatable = sum(c.NumGradientParams() > 0 for c in net.components)
        if len(scales) != num_updatable:
            raise SystemExit(f"{args.scales}: {len(scales)} scales for {num_updatable} "
                             "updatable components")
        net = net.Copy(scales=scales, remove_dropout=True)
        model = "test model (scaled, Dropout removed)"
    B = args.frames
    out_dim = net.components[-1].OutputDim()
    x = random_input(net, B)
    r = np.random.default_rng(20261019)
    labels = (np.arange(B, dtype=np.int32), r.integers(out_dim, size=B).astype(np.int32),
              np.ones(B, np.float32))

    def compute_prob(literal):
        def call():
            kcnn.set_literal_path(literal)
            try:
                net.ComputeProb(x, labels)
            finally:
                kcnn.set_literal_path(False)
        return call

    calls = {"compute_prob_fused": compute_prob(False),
             "compute_prob_literal": compute_prob(True),
             "propagate": lambda: net.Propagate(x)}
    net.ProbTotal(reset=True)
    ms = time_in_turn(calls, args.steps, args.warmup, torch.cuda.synchronize)
    objf, weight, acc = net.ProbTotal()
    b2b = time_back_to_back(calls, args.steps, 7, torch.cuda.synchronize)
    scopes = kernel_scopes(kcnn, calls, args.steps,
                           ("kn_softmax_prop", "kn_softmax_objf_accuracy", "kn_objf_accuracy"))
    out_bytes = B * out_dim * 4
    print(json.dumps({
        "metric": "ms_per_call", "workload": f"{os.path.basename(args.config)}, {model}",
        "components": net.NumComponents(), "frames_per_call": B, "steps": args.steps,
        "warmup": args.warmup,
        **{name: summary(v) for name, v in ms.items()},
        "back_to_back": {name: summary(v) for name, v in b2b.items()},
        "kernel_scope_ms": scopes,
        "frames_per_s_fused": round(B / (np.median(ms["compute_prob_fused"]) * 1e-3), 1),
        "output_bytes": out_bytes,
        "avg_logprob": objf / weight if weight else None,
        "accuracy": acc / weight if weight else None,
        "note": "host clock around one call and a device synchronise; the three are timed "
                "in turn; back_to_back: `steps` calls and one synchronise, 7 rounds in turn; "
                "kernel_scope_ms: hipEvent scopes (launch gaps included); output_bytes is "
                "what the fused path neither writes nor reads back"}))


if __name__ == "__main__":
    main()
