"""Training from labels on the reference's whole model (egs/exp/nnet/nnet.config,
kept byte for byte as tests/golden/nnet.config): 4096 frames a step, random
features, every step draws random labels and runs Propagate + BackpropXent
(Dropout masks drawn, Softmax + cross-entropy fused).  bench.py --config nnet
measures the same stack without its Dropout and Softmax layers and with a
synthetic output derivative; this is the step a user runs.

Prints one JSON line: frames_per_s, ms_per_step, the hipEvent-profile time of
the six kernels of nnet-loss-kernels.hip with their bandwidth on algorithmic
bytes (the four the step runs; kn_softmax_backprop and kn_comp_objf_and_deriv,
which only the literal path runs, timed alone on the step's shapes), and the
average log-probability per frame over the timed steps.  With --config
tests/golden/train_conv.config (the training recipes' topology) the line also
carries the two NormalizeComponent kernels and the share of the step their
scopes take.

  python scripts/nnet_xent_bench.py --steps 20 --warmup 5
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))

HBM_PEAK_GBS = 8000.0  # MI355X


def parse_profile(text):
    out = {}
    for line in text.strip().splitlines():
        parts = line.split("\t")
        if len(parts) >= 3:
            out[parts[0]] = (float(parts[1].split()[0]), int(parts[2].split()[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--config", default=os.path.join(ROOT, "tests", "golden", "nnet.config"))
    args = ap.parse_args()

    import torch
    import kcnn

    kcnn.init(0)
    net = kcnn.Nnet(open(args.config).read())
    B = args.frames
    out_dim = net.components[-1].OutputDim()
    context = sum(c._span() for c in net.components)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019)
    x = torch.randn(((context + 1) * B, net.components[0].InputDim()), generator=gen,
                    device="cuda")
    r = np.random.default_rng(20261019)
    rows = np.arange(B, dtype=np.int32)
    ones = np.ones(B, np.float32)

    def step():
        labels = (rows, r.integers(out_dim, size=B).astype(np.int32), ones)
        net.Propagate(x)
        net.BackpropXent(labels)

    def timed(profiled):
        kcnn.set_profiling(profiled)
        kcnn.reset_profile()
        net.ObjfTotal(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        kcnn.set_profiling(False)
        return el, parse_profile(kcnn.profile_string()) if profiled else {}, net.ObjfTotal()

    for _ in range(args.warmup):
        step()
    el, _, (objf, weight) = timed(False)
    _, prof, _ = timed(True)

    # the two kernels of the literal sequence, alone on the step's shapes
    sm = kcnn.Component.NewFromString(f"SoftmaxComponent dim={out_dim}")
    p = net.Output().clone()
    e = torch.randn(p.shape, generator=gen, device="cuda")
    d = torch.zeros_like(p)
    labels = (rows, r.integers(out_dim, size=B).astype(np.int32), ones)
    for profiled in (False, True):
        kcnn.set_profiling(profiled)
        kcnn.reset_profile()
        for _ in range(args.steps):
            sm.Backprop(None, p, e, in_deriv=d, update=True)
            kcnn.comp_objf_and_deriv(p, labels, d)
    kcnn.set_profiling(False)
    prof.update({k: v for k, v in parse_profile(kcnn.profile_string()).items()
                 if k in ("kn_softmax_backprop", "kn_comp_objf_and_deriv")})

    hidden = 4096
    for c in net.components:
        if c.Type() == "DropoutComponent":
            hidden = c.InputDim()
    passes = {  # matrix passes of algorithmic traffic, matrix width
        "kn_softmax_prop": (2, out_dim), "kn_softmax_xent_backprop": (2, out_dim),
        "kn_dropout_prop": (2, hidden), "kn_dropout_backprop": (4, hidden),
        "kn_softmax_backprop": (3, out_dim), "kn_comp_objf_and_deriv": (0, out_dim)}
    kernels = {}
    for name, (np_, width) in passes.items():
        if name not in prof:
            continue
        ms, calls = prof[name]
        per = ms / calls
        row = {"ms_per_call": round(per, 4), "calls": calls}
        if np_:
            gbs = np_ * B * width * 4 / (per * 1e-3) / 1e9
            row.update({"algorithmic_passes": np_, "GB/s": round(gbs, 1),
                        "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)})
        kernels[name] = row
    # NormalizeComponent layers (tests/golden/train_conv.config): one scope a
    # kernel over all of them, 2 passes forward and 3 backward per layer
    norm_dims = [c.InputDim() for c in net.components if c.Type() == "NormalizeComponent"]
    norm_ms = 0.0
    for name, np_ in (("kn_normalize_prop", 2), ("kn_normalize_backprop", 3)):
        if name not in prof:
            continue
        ms, calls = prof[name]
        norm_ms += ms
        gbs = np_ * B * sum(norm_dims) * 4 * (calls / len(norm_dims)) / (ms * 1e-3) / 1e9
        kernels[name] = {"ms_per_call": round(ms / calls, 4), "calls": calls,
                         "algorithmic_passes": np_, "GB/s": round(gbs, 1),
                         "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}
    print(json.dumps({
        "metric": "frames_per_s", "workload": f"{os.path.basename(args.config)} whole, Propagate + BackpropXent",
        "frames_per_step": B, "steps": args.steps, "warmup": args.warmup,
        "frames_per_s": round(B * args.steps / el, 1),
        "ms_per_step": round(el / args.steps * 1e3, 4),
        "kernels": kernels,
        **({"normalize_layers": norm_dims,
            "normalize_share_of_step": round(norm_ms / args.steps / (el / args.steps * 1e3), 4)}
           if norm_dims else {}),
        "avg_logprob": objf / weight if weight else None,
        "note": "kernel times are hipEvent scopes (launch gaps included); "
                "kn_softmax_backprop and kn_comp_objf_and_deriv are timed alone"}))


if __name__ == "__main__":
    main()
