"""Nnet.Compute with and without share_time on the workload of
scripts/compute_bench.py (profiles/compute.md): nnet.config's test model, 64
utterances of 200-600 frames drawn with the same seed (26438 frames), apply_log
and priors.  One pass a process, so that a run can use another build of the
library (KCNN_LIB) for the same call:

  python scripts/compute_shared_bench.py --pass own     # Compute as it stands
  python scripts/compute_shared_bench.py --pass shared  # share_time=True

A round is one call and one device synchronise; --warmup untimed rounds, then
--steps timed ones; reported: median [p10, p90], min, max.  Prints one JSON line.

--pass shared also compares, warm, against Compute of the same library:
Output(prefix - 1) of the two passes under the bound 2 E of
tests/test_gpu_compute_shared.py (E the 1e-5 S bar of each convolution
propagated in fp64 through the time maps, here on the device), and the
log-likelihoods and the posteriors by their largest difference; and reports the
activation floats below the first FC of either pass from the buffer sizes.
--no-check leaves the comparison out (a run under rocprofv3).  --kernels
instead runs --steps warm calls under the library's own per-function hipEvent
profile and prints it: the kernels of one call.  (Profiling synchronises around
every scope: not a call time.)

--config takes any network the plan covers, tests/golden/freq_conv.config (a
convolution along frequency: levels that keep a height) among them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from compute_bench import summary  # noqa: E402

RTOL = 1e-5


def error_bar(net, torch, lengths, prefix):
    """2 E at Output(prefix - 1) of the last shared pass, in the window layout."""
    left, right = net.LeftContext(), net.RightContext()
    context = left + right
    base = np.cumsum([0] + [t + context for t in lengths[:-1]])
    start = np.cumsum([0] + list(lengths[:-1]))
    views = [net.TimeMap(lvl) for lvl in range(prefix)]
    heights = [net.TimeMapHeight(lvl) for lvl in range(prefix)]
    err = torch.zeros(views[0][0].shape, dtype=torch.float64, device="cuda")
    for lvl in range(1, prefix):
        comp = net.components[lvl]
        a = views[lvl - 1][0].double()
        d_in = views[lvl - 1][3]
        rows = views[lvl][0].shape[0]
        kind = comp.Type()
        tall = heights[lvl] > 1 or (lvl > 1 and heights[lvl - 1] > 1)
        if kind == "ConvolutionComponent" and tall:
            # a level that keeps a height: column oh + g OH, weight row i + d kh + c kh kw
            w = comp.LinearParams().double().abs()
            h_in, c_in, oh = heights[lvl - 1], views[lvl - 1][1], heights[lvl]
            kh, g = h_in - oh + 1, w.shape[1]
            kw = w.shape[0] // (kh * c_in)
            s = comp.BiasParams().double().abs()[None, :, None].repeat(rows, 1, oh)
            e = torch.zeros_like(s)
            for c in range(c_in):
                for d in range(kw):
                    for i in range(kh):
                        wr = w[i + d * kh + c * kh * kw][None, :, None]
                        cols = slice(i + c * h_in, i + c * h_in + oh)
                        s += a[d_in * d:d_in * d + rows, cols].abs()[:, None, :] * wr
                        e += err[d_in * d:d_in * d + rows, cols][:, None, :] * wr
            err = (e + RTOL * s).reshape(rows, g * oh)
        elif kind == "ConvolutionComponent":
            w = comp.LinearParams().double().abs()
            width = a.shape[1]
            kw = w.shape[0] // width
            s = comp.BiasParams().double().abs().repeat(rows, 1)
            e = torch.zeros_like(s)
            for d in range(kw):
                wd = w[d * width:(d + 1) * width] if lvl == 1 else w[d::kw]
                s += a[d_in * d:d_in * d + rows].abs() @ wd
                e += err[d_in * d:d_in * d + rows] @ wd
            err = e + RTOL * s
        elif kind == "MaxpoolComponent" and heights[lvl - 1] > 1:
            h_in, c_in, c_out = heights[lvl - 1], views[lvl - 1][1], views[lvl][1]
            ph, pc, pw = h_in // heights[lvl], c_in // c_out, views[lvl][3] // d_in
            e3 = err.reshape(err.shape[0], c_in, h_in)
            err = torch.stack([e3[d_in * w:d_in * w + rows, c::pc, h::ph]
                               for c in range(pc) for w in range(pw)
                               for h in range(ph)]).amax(dim=0).reshape(rows, -1)
        elif kind == "MaxpoolComponent":
            c_out = views[lvl][1]
            pc = a.shape[1] // c_out
            pw = views[lvl][3] // d_in
            err = torch.stack([err[d_in * w:d_in * w + rows, c::pc]
                               for c in range(pc) for w in range(pw)]).amax(dim=0)
        else:
            err = err[:rows]
    _, c, n, d = views[-1]
    h = heights[-1]  # window layout: column h + k H + c H n
    bar = torch.empty((sum(lengths), c, n, h), dtype=torch.float64, device="cuda")
    for b, s0, t in zip(base, start, lengths):
        for k in range(n):
            bar[s0:s0 + t, :, k, :] = err[b + d * k:b + d * k + t].reshape(t, c, h)
    return 2.0 * bar.reshape(sum(lengths), c * n * h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pass", dest="which", choices=("own", "shared"), default="shared")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--min-frames", type=int, default=200)
    ap.add_argument("--max-frames", type=int, default=600)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--kernels", action="store_true")
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
    r = np.random.default_rng(args.seed)
    lengths = [int(t) for t in r.integers(args.min_frames, args.max_frames + 1,
                                          size=args.utterances)]
    frames = sum(lengths)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    x = torch.randn((frames, net.components[0].InputDim()), generator=gen, device="cuda")
    out_dim = net.components[-1].OutputDim()
    kw = {"apply_log": True, "priors": np.full(out_dim, 1.0 / out_dim, np.float32)}
    shared = args.which == "shared"
    if shared:
        kw["share_time"] = True

    if args.kernels:
        for _ in range(args.warmup):
            net.Compute(x, lengths, **kw)
        torch.cuda.synchronize()
        kcnn.reset_profile()
        kcnn.set_profiling(True)
        for _ in range(args.steps):
            net.Compute(x, lengths, **kw)
        torch.cuda.synchronize()
        kcnn.set_profiling(False)
        print(f"per-function hipEvent profile of {args.steps} warm calls (--pass {args.which}, "
              f"{len(lengths)} utterances, {frames} frames):")
        print(kcnn.profile_string())
        return 0

    ms = []
    for k in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.Compute(x, lengths, **kw)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    out = {"metric": "ms_per_call", "pass": args.which,
           "library": os.environ.get("KCNN_LIB") or "libkcnn.so",
           "workload": os.path.basename(args.config) + " test model",
           "utterances": len(lengths), "frames": frames, "steps": args.steps,
           "warmup": args.warmup, **summary(ms),
           "frames_per_s": round(frames / (np.median(ms) * 1e-3), 1)}
    if shared and not args.no_check:
        prefix = net.TimeSharedPrefix()
        ll = net.Compute(x, lengths, **kw).clone()
        top = net.Output(prefix - 1).double()
        bar = error_bar(net, torch, lengths, prefix)
        map_floats = sum(int(np.prod(net.TimeMap(lvl)[0].shape)) for lvl in range(1, prefix))
        map_floats += int(np.prod(net.Output(prefix - 1).shape))
        post = net.Output().clone()
        own_kw = {k: v for k, v in kw.items() if k != "share_time"}
        ll_own = net.Compute(x, lengths, **own_kw).clone()
        top_own = net.Output(prefix - 1).double()
        own_floats = sum(int(np.prod(net.Output(i).shape)) for i in range(prefix))
        post_own = net.Output().clone()
        diff = (top - top_own).abs()
        out.update({
            "prefix": prefix,
            "output_within_2E": bool((diff <= bar).all()),
            "worst_output_diff_over_2E": float((diff / bar.clamp_min(1e-300)).max()),
            "max_abs_diff_output": float(diff.max()),
            "max_abs_diff_loglikes": float((ll - ll_own).abs().max()),
            "max_abs_diff_posteriors": float((post - post_own).abs().max()),
            "largest_posterior": float(post_own.max()),
            "activation_floats_below_fc_shared": map_floats,
            "activation_floats_below_fc_own": own_floats,
            "gather_bytes": 2 * 4 * int(np.prod(net.Output(prefix - 1).shape))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
