"""Worker of tests/test_gpu_dp_xent.py, run under torch.distributed.run:
training from labels under data parallelism (kcnn_dp.dp_xent_step,
dp_train_epoch, dp_compute_prob_frames) through libkcnn.so on the GPU, with
gloo ranks sharing the device.  The network is a cut-down nnet.config.  Every
rank trains on its shards of the global minibatches; rank 0 then trains a fresh
replica with the same seeds on the whole minibatches in one process
(Propagate + BackpropXent, or kcnn.train_epoch).  Parameters and totals go to
<out>/rank<r>.npz and <out>/single.npz for the test to compare."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-cnn_amd"))
import kcnn      # noqa: E402
import kcnn_dp   # noqa: E402

D, CTX, G, PC, HID, OUT = 8, 2, 32, 4, 64, 12
W = 2 * CTX + 1
FC = ("FullyConnectedComponent input-dim={i} output-dim={o} learning-rate=0.02 "
      "param-stddev={s} bias-stddev=0.5 weight-decay=0.0002 momentum=0.9")
# Splice -> Conv -> Maxpool (a fused pair) -> ReLU -> Normalize -> FC -> ReLU ->
# Dropout -> FC -> Softmax
CFG = "\n".join([
    f"SpliceComponent input-dim={D} left-context={CTX} right-context={CTX} const-component-dim=0",
    f"ConvolutionComponent in-height={D} in-width={W} in-channel=1 kernel-height=3 "
    f"kernel-width=1 stride=1 group={G} out-height={D - 2} out-width={W} learning-rate=0.02 "
    "param-stddev=0.2 bias-stddev=0.5 weight-decay=0.0002 momentum=0.9",
    f"MaxpoolComponent in-height={D - 2} in-width={W} in-channel={G} pool-height-dim=1 "
    f"pool-width-dim=1 pool-channel-dim={PC}",
    f"RectifiedLinearComponent dim={(D - 2) * W * G // PC}",
    f"NormalizeComponent dim={(D - 2) * W * G // PC}",
    FC.format(i=(D - 2) * W * G // PC, o=HID, s=0.1),
    f"RectifiedLinearComponent dim={HID}",
    f"DropoutComponent dim={HID} dropout-proportion=0.5 dropout-scale=0.0",
    FC.format(i=HID, o=OUT, s=0.1),
    f"SoftmaxComponent dim={OUT}",
])
N_GLOBAL = (48, 37)                 # the steps' global minibatches: shards 24 / 24, 18 / 19
LENGTHS, MINIBATCH, SRAND = (20, 17, 12), 16, 3    # 49 rows: the last minibatch has one
HELD_OUT = (30, 7)


def new_net():
    """The same parameters and dropout seed every time."""
    kcnn.set_randn_seed(7)
    return kcnn.Nnet(CFG)


def state(net):
    out = {}
    for i, c in enumerate(net.components):
        if c.NumGradientParams() > 0:
            out[f"W{i}"] = c.LinearParams().cpu().numpy()
            out[f"b{i}"] = c.BiasParams().cpu().numpy()
            out[f"p{i}"] = c.PrevGrad().cpu().numpy()
    return out


def step_data():
    """Per step: the window matrix [n * W x D] and the labels (one per row,
    weights that do not sum to the row count)."""
    r = np.random.default_rng(11)
    out = []
    for n in N_GLOBAL:
        x = r.standard_normal((n * W, D)).astype(np.float32)
        cols = r.integers(0, OUT, size=n).astype(np.int32)
        weights = np.where(np.arange(n) % 3 == 0, 0.5, 1.0).astype(np.float32)
        out.append((x, cols, weights))
    return out


def corpora():
    r = np.random.default_rng(12)
    train = r.standard_normal((sum(LENGTHS), D)).astype(np.float32)
    pdfs = r.integers(0, OUT, size=sum(LENGTHS)).astype(np.int32)
    held = r.standard_normal((sum(HELD_OUT), D)).astype(np.float32)
    frames = r.permutation(sum(HELD_OUT)).astype(np.int32)
    labels = (np.arange(len(frames), dtype=np.int32),
              r.integers(0, OUT, size=len(frames)).astype(np.int32),
              np.where(np.arange(len(frames)) % 4 == 0, 0.25, 1.0).astype(np.float32))
    return train, pdfs, held, frames, labels


def run_steps(net, rank, world, grads):
    for x, cols, weights in step_data():
        n = len(cols)
        lo, hi = kcnn_dp.shard(n, world, rank)
        labels = (np.arange(hi - lo, dtype=np.int32), cols[lo:hi], weights[lo:hi])
        kcnn_dp.dp_xent_step(net, torch.from_numpy(x[lo * W:hi * W]).cuda(), labels, grads,
                             dist, n, lo)
    return {"objf": np.array(kcnn_dp.dp_objf_total(net, dist, reset=True))}


def single_steps(ref):
    for x, cols, weights in step_data():
        ref.Propagate(torch.from_numpy(x).cuda())
        ref.BackpropXent((np.arange(len(cols), dtype=np.int32), cols, weights))
    return {"objf": np.array(ref.ObjfTotal(reset=True))}


def run_epoch(net, grads):
    train, pdfs, held, frames, labels = corpora()
    corpus = kcnn.Corpus(torch.from_numpy(train).cuda(), list(LENGTHS))
    epoch = kcnn_dp.dp_train_epoch(net, corpus, pdfs, MINIBATCH, SRAND, dist, grads)
    held_out = kcnn.Corpus(torch.from_numpy(held).cuda(), list(HELD_OUT))
    kcnn_dp.dp_compute_prob_frames(net, held_out, frames, labels, dist)
    return {"objf": np.array(epoch), "prob": np.array(kcnn_dp.dp_prob_total(net, dist, True))}


def single_epoch(ref):
    train, pdfs, held, frames, labels = corpora()
    corpus = kcnn.Corpus(torch.from_numpy(train).cuda(), list(LENGTHS))
    epoch = kcnn.train_epoch(ref, corpus, pdfs, MINIBATCH, SRAND)
    held_out = kcnn.Corpus(torch.from_numpy(held).cuda(), list(HELD_OUT))
    ref.ComputeProbFrames(held_out, frames, labels)
    return {"objf": np.array(epoch), "prob": np.array(ref.ProbTotal(reset=True))}


def main():
    out_dir, what, backend = sys.argv[1], sys.argv[2], sys.argv[3]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if backend == "nccl":
        # RCCL: one GPU per rank (the one-GPU test box runs world size 1)
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{rank}"))
        kcnn.init(rank)
    else:
        dist.init_process_group("gloo")
        kcnn.init(0)
    net = new_net()
    if rank != 0:  # sync_dropout has something to do
        for c in net.components:
            if c.Type() == "DropoutComponent":
                c.SetDropoutSeed(1000 + rank)
    kcnn_dp.sync_dropout(net, dist)
    grads = kcnn_dp.gradient_buffers(net, lambda n: torch.empty(n, device="cuda"))
    totals = run_steps(net, rank, world, grads) if what == "steps" else run_epoch(net, grads)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **state(net), **totals)
    if rank == 0:
        ref = new_net()
        totals = single_steps(ref) if what == "steps" else single_epoch(ref)
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, "single.npz"), **state(ref), **totals)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
