"""Training from labels under data parallelism on the reference's whole model
(tests/golden/nnet.config): the step of scripts/nnet_xent_bench.py -- random
features, random labels drawn every step, Dropout masks drawn, Softmax +
cross-entropy fused -- run as kcnn_dp.dp_xent_step on every rank's shard of
--frames-per-gpu frames, the gradients all-reduced and the update applied with
the global frame count.  Run under torchrun, one rank per GPU (RCCL):

  torchrun --nproc-per-node 8 scripts/dp_xent_bench.py --steps 20 --warmup 5

World size 1 (also without torchrun) measures what the data-parallel form of
the step costs over Propagate + BackpropXent: the separate gradient and update
passes, the collectives' launches and the stream waits.

Rank 0 prints one JSON line: frames_per_s over all ranks, ms_per_step, and
from a second, marked pass the time the compute stream waited for the
all-reduces at the end of each step (what the overlap did not hide) as
ms and as a share of the step, next to the same collectives run alone.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames-per-gpu", type=int, default=4096)
    ap.add_argument("--config", default=os.path.join(ROOT, "tests", "golden", "nnet.config"))
    ap.add_argument("--dist-backend", default="nccl")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    import kcnn
    import kcnn_dp

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", rank))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    device = local if args.dist_backend == "nccl" else 0  # gloo ranks may share a GPU
    torch.cuda.set_device(device)
    if args.dist_backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world,
                                device_id=torch.device(f"cuda:{device}"))
    else:
        dist.init_process_group(args.dist_backend, rank=rank, world_size=world)
    kcnn.init(device)
    kcnn.set_randn_seed(20261020)  # identical replicas
    net = kcnn.Nnet(open(args.config).read())
    kcnn_dp.sync_dropout(net, dist)
    grads = kcnn_dp.gradient_buffers(net, lambda n: torch.empty(n, device="cuda"))

    B = args.frames_per_gpu
    lo, hi = kcnn_dp.shard(B * world, world, rank)
    out_dim = net.components[-1].OutputDim()
    context = sum(c._span() for c in net.components)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019 + rank)  # each rank its own shard of frames
    x = torch.randn(((context + 1) * B, net.components[0].InputDim()), generator=gen,
                    device="cuda")
    r = np.random.default_rng(20261019 + rank)
    rows = np.arange(B, dtype=np.int32)
    ones = np.ones(B, np.float32)
    marks = []
    marking = [False]

    def mark(name):
        if marking[0]:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

    def step():
        labels = (rows, r.integers(out_dim, size=B).astype(np.int32), ones)
        kcnn_dp.dp_xent_step(net, x, labels, grads, dist, B * world, lo, mark=mark)

    def timed():
        kcnn_dp.dp_objf_total(net, dist, reset=True)
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return el, kcnn_dp.dp_objf_total(net, dist)

    for _ in range(args.warmup):
        step()
    el, (objf, weight) = timed()
    marking[0] = True
    el_marked, _ = timed()
    marking[0] = False
    exposed = [b.elapsed_time(e) for (nb, b), (ne, e) in zip(marks[0::2], marks[1::2])
               if nb == "wait_begin" and ne == "wait_end"]
    exposed_ms = sum(exposed) / max(1, len(exposed))

    # the same collectives back to back with nothing else running
    bufs = [grads[i] for i in grads.large] + ([grads.bucket] if grads.bucket is not None else [])
    for b in bufs:
        dist.all_reduce(b)
    torch.cuda.synchronize()
    dist.barrier()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 5
    t0.record()
    for _ in range(reps):
        for b in bufs:
            dist.all_reduce(b)
    t1.record()
    torch.cuda.synchronize()
    alone_ms = t0.elapsed_time(t1) / reps

    ms_step = el / args.steps * 1e3
    if rank == 0:
        print(json.dumps({
            "metric": "frames_per_s",
            "workload": f"{os.path.basename(args.config)} whole, dp_xent_step",
            "world_size": world, "backend": dist.get_backend(),
            "frames_per_gpu": B, "global_batch": B * world,
            "steps": args.steps, "warmup": args.warmup,
            "frames_per_s": round(B * world * args.steps / el, 1),
            "ms_per_step": round(ms_step, 4),
            "ms_per_step_marked": round(el_marked / args.steps * 1e3, 4),
            "collectives_per_step": grads.num_collectives(),
            "allreduce_bytes_per_step": grads.bytes_per_step(),
            "allreduce_alone_ms_per_step": round(alone_ms, 4),
            "allreduce_exposed_ms_per_step": round(exposed_ms, 4),
            "allreduce_exposed_share_of_step": round(exposed_ms / ms_step, 4),
            "avg_logprob": objf / weight if weight else None,
            "note": "exposed = the compute stream's wait for the step's all-reduces at the "
                    "end of the backward (rank 0, marked pass); alone = the same collectives "
                    "back to back with nothing else running"}))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
