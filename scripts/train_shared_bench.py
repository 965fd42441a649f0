"""A training step with the convolutional prefix run once per time step:
Nnet.PropagateFrames(share_time=True) + BackpropXent beside the default
PropagateFrames + BackpropXent, on the same frame lists.

tests/golden/nnet.config at 512 frames a step, in two shapes: 32 runs of 16
consecutive corpus rows and 8 runs of 64 (the runs drawn, seeded, from a corpus
of --utts utterances of 100 to 700 frames).  Per shape two copies of one
network take turns in one process: after --warmup steps of each, `rounds`
times in turn --steps steps are enqueued one after the other with one device
synchronise, and the host clock gives ms per step.  The spread is the largest
less the smallest round of the default step.  Also printed: the rows each
level holds in both passes (the default pass: 512 windows x the level's
positions; the shared pass: the rows of the level's time map).  Prints one JSON
line a shape.

  python scripts/train_shared_bench.py --steps 20 --warmup 5

With --profile SHAPE (0 or 1) only that shape's shared step runs, --steps
times after the warm-up: the run to put under `rocprofv3 --kernel-trace
--stats` for the kernel statistics of a step.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))

SHAPES = [(32, 16), (8, 64)]  # (runs, frames a run): 512 frames a step


def draw_runs(r, starts, num_runs, k):
    """`num_runs` runs of k consecutive rows, each inside one utterance."""
    frames = []
    for _ in range(num_runs):
        u = int(r.integers(0, len(starts) - 1))
        first = int(r.integers(starts[u], starts[u + 1] - k + 1))
        frames.append(np.arange(first, first + k, dtype=np.int32))
    return np.concatenate(frames)


def series(ms):
    return [round(float(v), 4) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--profile", type=int, default=None)
    args = ap.parse_args()

    import torch
    import kcnn

    kcnn.init(0)
    config = open(os.path.join(ROOT, "tests", "golden", "nnet.config")).read()
    r = np.random.default_rng(20261021)
    lengths = r.integers(100, 701, size=args.utts).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    sync = torch.cuda.synchronize
    shapes = SHAPES if args.profile is None else [SHAPES[args.profile]]
    for num_runs, k in shapes:
        kcnn.set_randn_seed(20261021)
        nets = {"default": kcnn.Nnet(config), "shared": kcnn.Nnet(config)}
        d, out_dim = nets["default"].components[0].InputDim(), nets["default"].components[-1].OutputDim()
        feats = torch.from_numpy(r.standard_normal((int(starts[-1]), d)).astype(np.float32)).cuda()
        corpus = kcnn.Corpus(feats, lengths)
        frames = draw_runs(r, starts, num_runs, k)
        n = len(frames)
        labels = (np.arange(n, dtype=np.int32), r.integers(out_dim, size=n).astype(np.int32),
                  np.ones(n, np.float32))

        def step(name):
            nets[name].PropagateFrames(corpus, frames, share_time=name == "shared")
            nets[name].BackpropXent(labels)

        names = ["shared"] if args.profile is not None else ["default", "shared"]
        for _ in range(args.warmup):
            for name in names:
                step(name)
        sync()
        if args.profile is not None:
            for _ in range(args.steps):
                step("shared")
            sync()
            print(json.dumps({"profiled": "shared step", "runs": num_runs, "frames_a_run": k,
                              "steps": args.steps, "warmup": args.warmup}))
            continue
        ms = {name: [] for name in names}
        for _ in range(args.rounds):
            for name in names:
                sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(name)
                sync()
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        prefix = nets["shared"].TimeSharedTrainPrefix()
        levels = [nets["shared"].TimeMap(l) for l in range(prefix)]
        a, b = np.asarray(ms["default"]), np.asarray(ms["shared"])
        print(json.dumps({
            "metric": "ms_per_step", "workload": "nnet.config", "frames_per_step": n,
            "runs": num_runs, "frames_a_run": k, "prefix": prefix,
            "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup,
            "default_ms": series(a), "shared_ms": series(b),
            "default_median_ms": round(float(np.median(a)), 4),
            "shared_median_ms": round(float(np.median(b)), 4),
            "default_spread_ms": round(float(a.max() - a.min()), 4),
            "shared_over_default": round(float(np.median(b) / np.median(a)), 4),
            "rows_per_level_default": [n * lv[2] for lv in levels],
            "rows_per_level_shared": [int(lv[0].shape[0]) for lv in levels],
            "note": "host clock around `steps` steps and one device synchronise, the two steps "
                    "in turn, `rounds` times; spread: max - min of the default step's rounds"}))


if __name__ == "__main__":
    main()
