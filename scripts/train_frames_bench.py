"""A training step fed from a device-resident corpus: Nnet.PropagateFrames +
BackpropXent on a minibatch of corpus row indices, beside today's step on
window matrices.

For each config (default tests/golden/nnet.config and tests/golden/
train_conv.config) at --frames examples (default 4096) three steps are timed:

  a  Propagate on the examples' window matrix, already on the device, then
     BackpropXent: today's step, the floor.
  b  PropagateFrames on the examples' corpus rows, then BackpropXent.
  c  what a caller must do today: build the window matrix in numpy from the
     host copy of the corpus, copy it to the device, then a.

The corpus is --utts utterances of 100 to 700 frames (seeded), the examples a
seeded draw of its rows; a, b and c train on the same examples with the same
labels.  a and b alternate in one process: `rounds`, --rounds times in turn,
--steps steps enqueued one after the other and one device synchronise, ms per
step.  The spread of a is the largest less the smallest of its rounds; b
holds its bar when its median is no more than that spread above a's median.
c is timed the same way with fewer steps (its numpy build dominates) and has
no bar.  `gather_kernel_ms` is the hipEvent scope (launch gap included) of
kn_splice_frames_prop per step; run under `rocprofv3 --kernel-trace --stats`
for the kernel times themselves (splice_frames_kernel in b; splice_prop_kernel
and splice_backprop_kernel in a).  Prints one JSON line a config.

  python scripts/train_frames_bench.py --steps 20 --warmup 5
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))


def host_windows(feats, starts, frames, left, right):
    """The window matrix of the examples, in numpy: example n's rows
    clamp(r + o, s, e - 1), o = -left .. right."""
    utt = np.searchsorted(starts, frames, side="right") - 1
    idx = np.clip(frames[:, None] + np.arange(-left, right + 1)[None, :],
                  starts[utt][:, None], starts[utt + 1][:, None] - 1)
    return feats[idx.ravel()]


def rounds_in_turn(calls, steps, rounds, sync):
    """`steps` calls enqueued one after the other and one sync(), `rounds`
    times in turn; returns {name: ms per call of each round}."""
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, (fn, div) in calls.items():
            n = max(1, steps // div)
            sync()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            sync()
            ms[name].append((time.perf_counter() - t0) * 1e3 / n)
    return ms


def kernel_scopes(kcnn, fn, steps, keys):
    out = {}
    kcnn.set_profiling(True)
    try:
        kcnn.reset_profile()
        for _ in range(steps):
            fn()
        for line in kcnn.profile_string().strip().splitlines():
            parts = line.split("\t")
            if len(parts) >= 3 and parts[0] in keys:
                out[parts[0]] = round(float(parts[1].split()[0]) / steps, 4)
    finally:
        kcnn.set_profiling(False)
        kcnn.reset_profile()
    return out


def series(ms):
    return [round(float(v), 4) for v in ms]


def bench(kcnn, torch, config, args):
    kcnn.set_randn_seed(20261020)
    nets = {k: kcnn.Nnet(open(config).read()) for k in "abc"}
    net = nets["a"]
    left, right = net.LeftContext(), net.RightContext()
    d, out_dim = net.components[0].InputDim(), net.components[-1].OutputDim()
    r = np.random.default_rng(20261020)
    lengths = r.integers(100, 701, size=args.utts).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    feats = r.standard_normal((int(starts[-1]), d)).astype(np.float32)
    B = args.frames
    frames = r.integers(0, int(starts[-1]), size=B).astype(np.int32)
    labels = (np.arange(B, dtype=np.int32), r.integers(out_dim, size=B).astype(np.int32),
              np.ones(B, np.float32))
    dfeats = torch.from_numpy(feats).cuda()
    corpus = kcnn.Corpus(dfeats, lengths)
    win = torch.from_numpy(host_windows(feats, starts, frames, left, right)).cuda()

    def step_a():
        nets["a"].Propagate(win)
        nets["a"].BackpropXent(labels)

    def step_b():
        nets["b"].PropagateFrames(corpus, frames)
        nets["b"].BackpropXent(labels)

    def step_c():
        w = torch.from_numpy(host_windows(feats, starts, frames, left, right)).cuda()
        nets["c"].Propagate(w)
        nets["c"].BackpropXent(labels)

    sync = torch.cuda.synchronize
    for _ in range(args.warmup):
        step_a(), step_b(), step_c()
    sync()
    ms = rounds_in_turn({"a": (step_a, 1), "b": (step_b, 1), "c": (step_c, 4)}, args.steps,
                        args.rounds, sync)
    a, b, c = (np.asarray(ms[k]) for k in "abc")
    spread = float(a.max() - a.min())
    excess = float(np.median(b) - np.median(a))
    gather = kernel_scopes(kcnn, step_b, args.steps, ("kn_splice_frames_prop",))
    sync()
    print(json.dumps({
        "metric": "ms_per_step", "workload": os.path.basename(config), "frames_per_step": B,
        "corpus_rows": int(starts[-1]), "utterances": int(args.utts), "context": [left, right],
        "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup,
        "a_propagate_windows": series(a), "b_propagate_frames": series(b),
        "c_host_windows_copy_propagate": series(c),
        "a_median_ms": round(float(np.median(a)), 4), "b_median_ms": round(float(np.median(b)), 4),
        "c_median_ms": round(float(np.median(c)), 4), "a_spread_ms": round(spread, 4),
        "b_minus_a_ms": round(excess, 4), "b_within_a_spread": bool(excess <= spread),
        "frames_per_s": {k: round(B / (float(np.median(v)) * 1e-3), 1)
                         for k, v in (("a", a), ("b", b), ("c", c))},
        "gather_kernel_ms": gather,
        "window_matrix_bytes": int(win.numel() * 4), "example_triple_bytes": 12 * B,
        "note": "host clock around `steps` steps and one device synchronise, a, b and c in "
                "turn, `rounds` times (c: steps / 4); spread: max - min of a's rounds; "
                "kernel scopes: hipEvent scopes per step, launch gaps included"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--config", action="append",
                    help="a network config (may be given more than once)")
    args = ap.parse_args()
    configs = args.config or [os.path.join(ROOT, "tests", "golden", n)
                              for n in ("nnet.config", "train_conv.config")]

    import torch
    import kcnn

    kcnn.init(0)
    for config in configs:
        bench(kcnn, torch, config, args)


if __name__ == "__main__":
    main()
