"""The whole-utterance forward pass, Nnet.Compute (upstream NnetComputer:
nnet-am-compute, the decodable), on nnet.config's test model: frames/s of

  1. compute_batch:   Compute on a batch of utterances in one pass (default 64
                      utterances of 200-600 frames, uniform, fixed seed);
  2. propagate_windows: Propagate on the same frames as prebuilt windows, one
                      21-frame window per frame (what a caller had to build
                      and upload before Compute existed; the upload is not
                      timed, only the 21x input the first Splice reads);
  3. compute_single:  Compute one utterance at a time, the same utterances.

All three produce the posteriors of the same frames.  A round of a case is
all its calls enqueued one after the other and one device synchronise.  The
cases are timed in blocks, a case's --warmup rounds and then its --steps
timed rounds, and the three blocks are run twice over (a b c a b c) so that a
drift of the machine shows: the stack sizes its activations for the row count
of a call, so rounds of different cases taken in turn would each pay the
other's re-sizing, which a loop over one kind of call does not (case 3, whose
utterances differ in length, pays it in every call, as it would in use).
Reported per case: the median round with its minimum, maximum and 10th /
90th percentiles, over both blocks.  Compute runs with apply_log and priors
(the decodable's log-likelihoods); --no-log times the plain posteriors.
Prints one JSON line.

--splice-only instead times the two Splice kernels alone on the shape of
nnet.config's first layer (dim 40, 21 slots, --frames output rows): the
whole-utterance kernel on [frames x 40] utterance rows and kn_splice_prop on
the [frames * 21 x 40] window input; both write frames x 840 floats.  Run it
under `rocprofv3 --kernel-trace --stats` for the kernel times (splice_ragged_
kernel / splice_prop_kernel); the JSON line gives the bytes stored per call.

  python scripts/compute_bench.py --steps 20 --warmup 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))


def summary(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4), "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4)}


def time_in_blocks(calls, steps, warmup, sync, repeats=2):
    """calls: {name: function}.  `repeats` times over, each function in a
    block of its own: `warmup` untimed rounds, then `steps` timed ones, each
    between two sync()s.  Returns {name: ms of each timed round}."""
    ms = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            for k in range(warmup + steps):
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                if k >= warmup:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def window_index(lengths, left, right):
    """Row indices into the stacked utterances of every frame's clamped window."""
    idx, start = [], 0
    for t in lengths:
        f = np.arange(t)[:, None] + np.arange(-left, right + 1)[None, :]
        idx.append(start + np.clip(f, 0, t - 1).reshape(-1))
        start += t
    return np.concatenate(idx)


def splice_only(args, kcnn, torch):
    net = kcnn.Nnet("SpliceComponent input-dim=40 left-context=10 right-context=10 "
                    "const-component-dim=0")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261020)
    rows = args.frames
    lengths = [rows // 8] * 7 + [rows - 7 * (rows // 8)]
    x = torch.randn((rows, 40), generator=gen, device="cuda")
    win = x[torch.from_numpy(window_index(lengths, 10, 10)).cuda()].contiguous()
    net.Propagate(win)
    want = net.Output().clone()
    same = bool(torch.equal(net.Compute(x, lengths), want))
    for _ in range(args.warmup + args.steps):  # alternating: the same machine for both
        net.Compute(x, lengths)
        net.Propagate(win)
    torch.cuda.synchronize()
    print(json.dumps({"mode": "splice-only", "rows": rows, "dim": 40, "slots": 21,
                      "utterances": len(lengths), "calls_each": args.warmup + args.steps,
                      "bytes_stored_per_call": rows * 840 * 4,
                      "bytes_read_ragged": rows * 40 * 4, "bytes_read_windows": rows * 840 * 4,
                      "outputs_bit_identical": same}))
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--min-frames", type=int, default=200)
    ap.add_argument("--max-frames", type=int, default=600)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--no-log", action="store_true")
    ap.add_argument("--splice-only", action="store_true")
    ap.add_argument("--frames", type=int, default=4096, help="--splice-only: output rows")
    ap.add_argument("--config", default=os.path.join(ROOT, "tests", "golden", "nnet.config"))
    ap.add_argument("--scales", default=os.path.join(ROOT, "tests", "golden",
                                                     "dropout_scale.config"))
    args = ap.parse_args()

    import torch
    import kcnn

    kcnn.init(0)
    if args.splice_only:
        return splice_only(args, kcnn, torch)
    kcnn.set_randn_seed(args.seed)
    net = kcnn.Nnet(open(args.config).read())
    net.components[-2].PerturbParams(0.05)  # nnet.config's last FC starts at zero
    if any(c.Type() == "DropoutComponent" for c in net.components):
        scales = [float(s) for s in open(args.scales).read().strip().split(":")]
        net = net.Copy(scales=scales, remove_dropout=True)
    left, right = net.LeftContext(), net.RightContext()
    r = np.random.default_rng(args.seed)
    lengths = [int(t) for t in r.integers(args.min_frames, args.max_frames + 1,
                                          size=args.utterances)]
    frames = sum(lengths)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    x = torch.randn((frames, net.components[0].InputDim()), generator=gen, device="cuda")
    win = x[torch.from_numpy(window_index(lengths, left, right)).cuda()].contiguous()
    singles = list(torch.split(x, lengths))
    out_dim = net.components[-1].OutputDim()
    kw = {} if args.no_log else {"apply_log": True,
                                 "priors": np.full(out_dim, 1.0 / out_dim, np.float32)}

    def compute_single():
        for u in singles:
            net.Compute(u, **kw)

    calls = {"compute_batch": lambda: net.Compute(x, lengths, **kw),
             "propagate_windows": lambda: net.Propagate(win),
             "compute_single": compute_single}
    ms = time_in_blocks(calls, args.steps, args.warmup, torch.cuda.synchronize)
    # the cases compute the same posteriors (compared warm: both have run)
    net.Propagate(win)
    p = net.Output().clone()
    q = net.Compute(x, lengths)
    same = bool(torch.equal(p.view(torch.int32), q.view(torch.int32)))
    max_diff = float((p - q).abs().max())
    print(json.dumps({
        "metric": "frames_per_s", "workload": os.path.basename(args.config) + " test model",
        "utterances": len(lengths), "frames": frames, "min_frames": min(lengths),
        "max_frames": max(lengths), "seed": args.seed, "left_context": left,
        "right_context": right, "apply_log_and_priors": not args.no_log,
        "steps": args.steps, "warmup": args.warmup,
        **{name: summary(v) for name, v in ms.items()},
        **{"frames_per_s_" + name: round(frames / (np.median(v) * 1e-3), 1)
           for name, v in ms.items()},
        "input_bytes_compute": frames * x.shape[1] * 4,
        "input_bytes_windows": int(win.shape[0]) * x.shape[1] * 4,
        "posteriors_bit_identical_batch_vs_windows": same,
        "max_abs_diff_batch_vs_windows": max_diff,
        "note": "host clock around one round (all the calls of the case, one device "
                "synchronise); each case in blocks of its own, twice over; "
                "propagate_windows leaves out building and uploading the windows and "
                "computes no log-likelihoods"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
