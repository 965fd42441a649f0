"""The streaming forward pass, OnlineComputer.Accept (upstream
NnetOnlineComputer: the decodable of online2-wav-nnet2-latgen-faster), on
nnet.config's test model in steady state: --streams utterances (default 32),
each given --chunk new frames a step (default 16), none ending.  Per case, ms
per step and frames/s of

  1. online_accept:  one Accept a step over all the streams;
  2. cat_compute:    what a caller could do before OnlineComputer existed: a
                     kept history of L + R frames per stream, torch.cat of it
                     and the stream's chunk, torch.cat of the streams, one
                     Compute(..., pad_input=False), and the new history sliced
                     off (the utterance edges, which that route leaves to the
                     caller, do not occur in steady state);
  3. compute_whole:  Compute on the frames of a round as whole utterances
                     (--streams utterances of chunk x steps-per-round frames,
                     one call a round): what the step granularity costs.

The cases produce the log-likelihoods of the same frames; the largest
difference between Accept's rows of fresh streams and Compute without padding
on the same streams whole (what the cat route's calls add up to) is reported,
not judged: tests/test_gpu_online.py holds the bar.  A round of a case is
--steps-per-round steps enqueued one after the other and one device
synchronise; the cases are timed in blocks, twice over, as
scripts/compute_bench.py times its cases.  Prints one JSON line.

--kernels instead runs --steps steady-state steps of Accept under the
library's own per-function hipEvent profile and prints it: the kernels of one
step.  (Profiling synchronises around every scope: not a step time.)

--share-time makes every computer with share_time=True (the leading Splice ->
Convolution / Maxpool / ReLU components once per time step of the frames the
slots hold), also under --kernels, and reports the largest
difference of its log-likelihoods from the default computer's on the same
steps.

  python scripts/online_compute_bench.py --steps 20 --warmup 3
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from compute_bench import summary, time_in_blocks  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed rounds per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--steps-per-round", type=int, default=8)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--no-log", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--share-time", action="store_true")
    ap.add_argument("--config", default=os.path.join(ROOT, "tests", "golden", "nnet.config"))
    ap.add_argument("--scales", default=os.path.join(ROOT, "tests", "golden",
                                                     "dropout_scale.config"))
    args = ap.parse_args()

    import torch
    import kcnn

    kcnn.init(0)
    kcnn.set_randn_seed(args.seed)
    net = kcnn.Nnet(open(args.config).read())
    net.components[-2].PerturbParams(0.05)  # nnet.config's last FC starts at zero
    if any(c.Type() == "DropoutComponent" for c in net.components):
        scales = [float(s) for s in open(args.scales).read().strip().split(":")]
        net = net.Copy(scales=scales, remove_dropout=True)
    left, right = net.LeftContext(), net.RightContext()
    n, c, spr = args.streams, args.chunk, args.steps_per_round
    d, out_dim = net.components[0].InputDim(), net.components[-1].OutputDim()
    kw = {} if args.no_log else {"apply_log": True,
                                 "priors": np.full(out_dim, 1.0 / out_dim, np.float32)}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    # a round's frames, [stream, frame, column]; every round feeds them again
    # (the values do not matter to the time, and the streams never end)
    pool = torch.randn((n, c * spr, d), generator=gen, device="cuda")
    chunks = [pool[:, k * c:(k + 1) * c].reshape(n * c, d).contiguous() for k in range(spr)]
    per_stream = [[pool[s, k * c:(k + 1) * c] for s in range(n)] for k in range(spr)]
    whole = pool.reshape(n * c * spr, d)
    slots, num_new, final = list(range(n)), [c] * n, [False] * n

    def new_online():
        if args.share_time:
            return kcnn.OnlineComputer(net, n, c, share_time=True, **kw)
        return kcnn.OnlineComputer(net, n, c, **kw)

    def new_history():
        return [torch.zeros((left + right, d), device="cuda") for _ in range(n)]

    def cat_step(hist, k):
        parts = [torch.cat((hist[s], per_stream[k][s])) for s in range(n)]
        out = net.Compute(torch.cat(parts), [left + right + c] * n, pad_input=False, **kw)
        for s in range(n):
            hist[s] = parts[s][c:]
        return out

    # ---- the routes compute the same frames: a stream's frames L .. T - R - 1
    # from Accept (fresh streams, none final) against Compute without padding
    # on the stream whole, which is what the cat route's calls add up to
    oc = new_online()
    got = [[] for _ in range(n)]
    for k in range(spr):
        out, counts = oc.Accept(chunks[k], slots, num_new, final)
        for s, rows in enumerate(torch.split(out, counts)):
            got[s].append(rows.clone())
    worst = None
    if c * spr > left + right:
        want = net.Compute(whole, [c * spr] * n, pad_input=False, **kw)
        streamed = torch.cat([torch.cat(g)[left:] for g in got])
        worst = float((streamed - want).abs().max())
    worst_shared = None
    if args.share_time:
        assert oc.TimeSharedPrefix() > 0, "the plan declines this network"
        own = kcnn.OnlineComputer(net, n, c, **kw)
        worst_shared = 0.0
        for k in range(spr):
            out, _ = own.Accept(chunks[k], slots, num_new, final)
            if out.shape[0]:
                theirs = torch.cat([g[k] for g in got])
                worst_shared = max(worst_shared, float((out - theirs).abs().max()))

    if args.kernels:
        oc = new_online()
        for k in range(args.warmup * spr):
            oc.Accept(chunks[k % spr], slots, num_new, final)
        torch.cuda.synchronize()
        kcnn.reset_profile()
        kcnn.set_profiling(True)
        for k in range(args.steps):
            oc.Accept(chunks[k % spr], slots, num_new, final)
        torch.cuda.synchronize()
        kcnn.set_profiling(False)
        print(f"per-function hipEvent profile of {args.steps} steady-state Accept steps "
              f"({n} streams x {c} frames{', share_time' if args.share_time else ''}):")
        print(kcnn.profile_string())
        return 0

    state = {"oc": new_online(), "hist": new_history()}

    def online_round():
        for k in range(spr):
            state["oc"].Accept(chunks[k], slots, num_new, final)

    def cat_round():
        for k in range(spr):
            cat_step(state["hist"], k)

    calls = {"online_accept": online_round, "cat_compute": cat_round,
             "compute_whole": lambda: net.Compute(whole, [c * spr] * n, **kw)}
    ms = time_in_blocks(calls, args.steps, args.warmup, torch.cuda.synchronize)
    frames = n * c * spr
    print(json.dumps({
        "metric": "ms_per_step", "workload": os.path.basename(args.config) + " test model",
        "streams": n, "chunk": c, "steps_per_round": spr, "frames_per_round": frames,
        "left_context": left, "right_context": right, "seed": args.seed,
        "apply_log_and_priors": not args.no_log, "steps": args.steps, "warmup": args.warmup,
        "share_time": args.share_time,
        **{name: summary(v) for name, v in ms.items()},
        **{"ms_per_step_" + name: round(float(np.median(v)) / spr, 4) for name, v in ms.items()},
        **{"frames_per_s_" + name: round(frames / (np.median(v) * 1e-3), 1)
           for name, v in ms.items()},
        "max_abs_diff_online_vs_unpadded_compute": worst,
        "max_abs_diff_shared_vs_default_computer": worst_shared,
        "note": "host clock around one round (steps_per_round steps, one device synchronise); "
                "each case in blocks of its own, twice over; compute_whole is one call a "
                "round on the round's frames as whole utterances (ms_per_step is that call "
                "over steps_per_round)"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
