"""NormalizeComponent's two kernels beside their Softmax twins (the same reads
and writes, the same row reductions) at one shape.

  python scripts/normalize_bench.py --cols 1152 [--rows 4096] [--reps 50] [--rounds 5]

Runs normalize prop / backprop and softmax prop / backprop (no statistics) in
turn, `rounds` times `reps` launches each, and prints one JSON line: HIP-event
microseconds a launch (the median round and the rounds' min / max; launch gaps
included, so short kernels read high) and GB/s on the algorithmic traffic
(8 * rows * cols bytes forward, 12 * rows * cols backward).  Kernel times come
from a `rocprofv3 --kernel-trace --stats` run of this script, one shape a run
(the kernel names do not carry the shape); `scripts/kstats.py` prints them.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))

import torch  # noqa: E402

import kcnn  # noqa: E402


def time_round(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--cols", type=int, required=True)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    kcnn.init(0)
    N, D = a.rows, a.cols
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019)
    norm = kcnn.Component.NewFromString(f"NormalizeComponent dim={D}")
    soft = kcnn.Component.NewFromString(f"SoftmaxComponent dim={D}")
    x = torch.randn((N, D), generator=gen, device="cuda")
    e = torch.randn((N, D), generator=gen, device="cuda")
    y, d = torch.empty_like(x), torch.empty_like(x)
    p = soft.Propagate(x)
    tests = {
        "normalize_prop": (lambda: norm.Propagate(x, out=y), 8),
        "softmax_prop": (lambda: soft.Propagate(x, out=y), 8),
        "normalize_backprop": (lambda: norm.Backprop(x, None, e, in_deriv=d, update=False), 12),
        "softmax_backprop": (lambda: soft.Backprop(None, p, e, in_deriv=d, update=False), 12),
    }
    for fn, _ in tests.values():  # warm-up: code objects loaded, clocks up
        for _ in range(a.reps):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in tests}
    for _ in range(a.rounds):  # the four in turn, so a drift touches all alike
        for name, (fn, _) in tests.items():
            us[name].append(time_round(fn, a.reps))
    out = {"rows": N, "cols": D, "reps": a.reps, "rounds": a.rounds, "events_us": {}}
    for name, (_, bytes_per_el) in tests.items():
        t = sorted(us[name])
        med = t[len(t) // 2]
        out["events_us"][name] = {
            "median": round(med, 2), "min": round(t[0], 2), "max": round(t[-1], 2),
            "GB/s": round(bytes_per_el * N * D / med / 1e3, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
