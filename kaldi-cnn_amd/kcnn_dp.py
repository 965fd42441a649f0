"""Data-parallel training step for a kcnn component stack.

One process per GPU (torch.distributed, backend "nccl" = RCCL on ROCm): the
minibatch is row-sharded -- frames are independent through Conv, Maxpool and
FC -- and every rank holds a full replica of the parameters.  The only
exchange is the parameter gradient, summed (fp32) by as few all-reduces as
the overlap allows:

  * every gradient shorter than SPLIT_GRADIENT_PARAMS values -- all the
    convolutions' filter and bias gradients (c2: 3,200 values; c5: four
    layers, 1.2 M) -- lives in ONE flat bucket and is reduced by one
    all-reduce once the last of them exists (north_star's single all-reduce
    of the filter/bias gradients);
  * a gradient at least that long (an FC layer's: 11.9 M values, 47.6 MB at
    c2) gets its own all-reduce, started as soon as that gradient is
    computed (kcnn_nnet_backprop_component mode 3) and before the layer's
    data gradient (mode 2), so it runs over xGMI beside the FC dX GEMM and
    the conv/maxpool backward below it.

So the c2 and c5 steps issue two collectives, nnet.config four (three FC
layers + the bucket).  Every replica then applies the reference's update
step (nnet-component-nnet0.cc:767-775) with the GLOBAL frame count, which
reproduces the single-GPU math at the same global batch (the reference
itself divides by its local row count, :767).

`net` is duck-typed: anything with NumComponents(), components[i]
(NumGradientParams, ApplyGradient), Propagate(x),
BackpropComponent(i, out_deriv, mode, grad) and BackpropSplit(i, out_deriv,
grad, skip_first_dx, between) -- kcnn.Nnet on the GPU; the tests drive the
same function with a CPU stand-in over gloo.

dp_train_step takes a caller's output derivative (the bench stacks).  The
steps from labels -- dp_xent_step, dp_xent_step_frames, dp_train_epoch --
train whole networks: SetRowOffset(shard start) makes a DropoutComponent draw
the masks of the GLOBAL rows, XentDeriv leaves the cross-entropy derivative
for the same per-component backward, and the objective totals are summed over
the ranks (dp_objf_total, dp_prob_total).  For these `net` also has
SetRowOffset(offset) and XentDeriv(labels) -> (first, out_deriv).
NonlinearComponent statistics stay per replica: each covers its own shard.
"""
from __future__ import annotations

import os

# gradients at least this long get their own all-reduce, started before the
# layer's data gradient; shorter ones share the flat bucket
SPLIT_GRADIENT_PARAMS = int(os.environ.get("KCNN_DP_SPLIT_PARAMS", 1 << 20))


class GradientBuffers:
    """A replica's gradient storage: {component index: flat [linear | bias]
    buffer}.  Components with fewer than `own` gradient values get views into
    one contiguous bucket (in component order); the others own a buffer."""

    def __init__(self, net, alloc, own=None):
        own = SPLIT_GRADIENT_PARAMS if own is None else own
        sizes = {i: c.NumGradientParams() for i, c in enumerate(net.components)
                 if c.NumGradientParams() > 0}
        self.large = sorted(i for i, n in sizes.items() if n >= own)
        self.small = sorted(i for i in sizes if i not in self.large)
        total = sum(sizes[i] for i in self.small)
        self.bucket = alloc(total) if total else None
        self.bufs = {}
        off = 0
        for i in self.small:
            self.bufs[i] = self.bucket[off:off + sizes[i]]
            off += sizes[i]
        for i in self.large:
            self.bufs[i] = alloc(sizes[i])

    def __contains__(self, i):
        return i in self.bufs

    def __getitem__(self, i):
        return self.bufs[i]

    def num_collectives(self):
        return len(self.large) + (1 if self.bucket is not None else 0)

    def bytes_per_step(self):
        return sum(b.numel() for b in self.bufs.values()) * 4


def gradient_buffers(net, alloc, own=None):
    return GradientBuffers(net, alloc, own)


def _backward_update(net, first, out_deriv, grads, dist, frames_global, mark=None):
    """The tail every step shares: the backward from component `first` down
    (None: this rank's shard is empty and no kernel of the network runs), each
    gradient's all-reduce, and the update with the global frame count.

    mode 1 = data gradient and parameter gradient (no update), mode 2 = data
    gradient only, mode 3 = parameter gradient only
    (kcnn_nnet_backprop_component).  The first layer's input derivative is
    computed too, as upstream NnetUpdater does and as the 1-GPU step
    (Nnet.Backprop) does, so N=1 and N>1 do the same work.

    The collectives and their order depend on `grads` alone, so a rank with
    an empty shard issues the same ones over zeroed buffers."""
    pending = []
    if first is None:
        for i in reversed(grads.large):
            grads[i].zero_()
            pending.append(([i], dist.all_reduce(grads[i], async_op=True)))
        if grads.bucket is not None:
            grads.bucket.zero_()
    for i in reversed(range(0 if first is None else first + 1)):
        if i in grads.large and getattr(net.components[i], "SplitGradient", lambda: True)():
            # the gradient, its all-reduce started, then the data gradient
            # (one library call: both GEMMs' statistics from one pass)
            def start(i=i):
                pending.append(([i], dist.all_reduce(grads[i], async_op=True)))
            net.BackpropSplit(i, out_deriv, grads[i], False, start)
        elif i in grads.large:
            net.BackpropComponent(i, out_deriv, mode=1, grad=grads[i], skip_first_dx=False)
            pending.append(([i], dist.all_reduce(grads[i], async_op=True)))
        elif i in grads:
            net.BackpropComponent(i, out_deriv, mode=1, grad=grads[i], skip_first_dx=False)
        else:
            net.BackpropComponent(i, out_deriv, mode=2, skip_first_dx=False)
    if grads.bucket is not None:
        pending.append((grads.small, dist.all_reduce(grads.bucket, async_op=True)))
    if mark:
        mark("wait_begin")
    # NCCL (RCCL) runs a process group's collectives in order on one stream,
    # so the compute stream waits for the last one alone: each stream wait
    # (and the event behind it) cost the c2 step 20-50 us of GPU idle at
    # world size 1 (rocprofv3 trace); other backends wait for each
    backend = getattr(dist, "get_backend", lambda: None)()
    waits = pending[-1:] if backend == "nccl" else pending
    for _, work in waits:
        work.wait()
    if mark:
        mark("wait_end")
    for ids, _ in pending:
        for i in ids:
            net.components[i].ApplyGradient(grads[i], frames_global)


def dp_train_step(net, x, out_deriv, grads, dist, frames_global, mark=None):
    """Propagate + backprop from a caller's output derivative + all-reduced
    update of one row shard (_backward_update from the last component).

    mark(name), when given, is called on the host at "wait_begin" (all
    collectives issued, the backward queued) and "wait_end" (the compute
    stream now waits for every collective): bench.py records stream events
    there to measure the all-reduce time the step did not hide."""
    net.Propagate(x)
    _backward_update(net, net.NumComponents() - 1, out_deriv, grads, dist, frames_global, mark)


def shard(n, world, rank):
    """Rank `rank`'s contiguous rows [lo, hi) of a global minibatch of n rows:
    the shards partition [0, n) and their sizes differ by at most one (a
    minibatch smaller than the world leaves some of them empty)."""
    return n * rank // world, n * (rank + 1) // world


def _xent_tail(net, forward, labels, grads, dist, frames_global, row_offset, mark):
    if forward is None:
        # An empty shard: no kernel of the network runs, but the dropout masks
        # of the ranks' next minibatch are those of one Propagate call number,
        # so this rank counts the call it did not make.
        getattr(net, "SkipDropoutCall", lambda: None)()
        _backward_update(net, None, None, grads, dist, frames_global, mark)
        return
    net.SetRowOffset(row_offset)
    forward()
    first, out_deriv = net.XentDeriv(labels)
    _backward_update(net, first, out_deriv, grads, dist, frames_global, mark)


def dp_xent_step(net, x, labels, grads, dist, frames_global, row_offset, mark=None):
    """One training step from labels on this rank's shard `x` of a global
    minibatch of `frames_global` rows, of which x's row 0 is row `row_offset`
    (shard()): dropout masks drawn for the global rows, Propagate, the
    cross-entropy derivative (Nnet.XentDeriv; the labels' rows are local to
    the shard), then _backward_update.  With the replicas' dropout seeds equal
    (sync_dropout) the masks are those one process draws on the whole
    minibatch.  frames_global is the ROW count of the global minibatch, not
    the labels' weight: the reference's Update divides by N.  A rank whose
    shard has no rows runs no kernel of the network; it zeroes its gradient
    buffers, joins the same collectives in the same order and applies the
    update, so the replicas stay identical."""
    forward = (lambda: net.Propagate(x)) if x.shape[0] > 0 else None
    _xent_tail(net, forward, labels, grads, dist, frames_global, row_offset, mark)


def dp_xent_step_frames(net, corpus, frames, labels, grads, dist, frames_global, row_offset,
                        mark=None):
    """dp_xent_step with Nnet.PropagateFrames as the forward: `frames` are
    this rank's shard of the global minibatch's corpus rows.  Every rank holds
    the whole corpus."""
    forward = (lambda: net.PropagateFrames(corpus, frames)) if len(frames) > 0 else None
    _xent_tail(net, forward, labels, grads, dist, frames_global, row_offset, mark)


def _host_device(dist):
    """Where the small host-side collectives live: RCCL reduces device
    tensors only."""
    return "cuda" if getattr(dist, "get_backend", lambda: None)() == "nccl" else "cpu"


def _dropouts(net):
    return [c for c in net.components
            if getattr(c, "Type", lambda: "")() == "DropoutComponent"]


def sync_dropout(net, dist):
    """Rank 0's dropout seeds to every replica.  SetDropoutSeed restarts the
    call count, so the counts agree too: call it once before training."""
    import numpy as np
    import torch
    drops = _dropouts(net)
    if not drops:
        return
    seeds = np.array([c.DropoutSeed() for c in drops], np.uint64)
    t = torch.from_numpy(seeds.view(np.int64).copy()).to(_host_device(dist))
    dist.broadcast(t, src=0)
    for c, s in zip(drops, t.cpu().numpy().view(np.uint64)):
        c.SetDropoutSeed(int(s))


def _all_reduced(values, dist):
    import torch
    t = torch.tensor(values, dtype=torch.float64, device=_host_device(dist))
    dist.all_reduce(t)
    return tuple(t.tolist())


def dp_objf_total(net, dist, reset=False):
    """Nnet.ObjfTotal (synchronises) summed over the ranks: (objective,
    weight) of the global minibatches since the last reset."""
    return _all_reduced(net.ObjfTotal(reset), dist)


def dp_prob_total(net, dist, reset=False):
    """Nnet.ProbTotal (synchronises) summed over the ranks."""
    return _all_reduced(net.ProbTotal(reset), dist)


def dp_compute_prob_frames(net, corpus, frames, labels, dist):
    """Evaluation under data parallelism: ComputeProbFrames on this rank's
    shard of `frames` (global corpus rows) and of `labels` ((rows, cols,
    weights) arrays, rows into `frames`, sorted by row); dp_prob_total sums
    the ranks' totals.  The components run as they are, so a DropoutComponent
    draws its mask, for the global rows as in training (evaluate the test
    model to have none).  An empty shard runs nothing."""
    import numpy as np
    rows, cols, weights = (np.asarray(a) for a in labels)
    frames = np.asarray(frames)
    lo, hi = shard(len(frames), dist.get_world_size(), dist.get_rank())
    if hi == lo:
        getattr(net, "SkipDropoutCall", lambda: None)()
        return
    net.SetRowOffset(lo)
    keep = (rows >= lo) & (rows < hi)
    net.ComputeProbFrames(corpus, frames[lo:hi], (rows[keep] - lo, cols[keep], weights[keep]))


def dp_train_epoch(net, corpus, pdfs, minibatch_size, srand, dist, grads):
    """kcnn.train_epoch under data parallelism: every rank draws the same
    numpy permutation of all corpus rows seeded by `srand`, takes its shard()
    of every global minibatch (row_offset = the shard's start) and runs
    dp_xent_step_frames with the minibatch's row count.  Returns the
    all-reduced (objf, frames) of dp_objf_total(reset=True)."""
    import numpy as np
    pdfs = np.ascontiguousarray(pdfs, np.int32).ravel()
    rows = corpus.NumRows()
    if len(pdfs) != rows:
        raise ValueError(f"dp_train_epoch: {len(pdfs)} pdfs for a corpus of {rows} rows")
    if minibatch_size < 1:
        raise ValueError(f"dp_train_epoch: minibatch_size {minibatch_size}")
    world, rank = dist.get_world_size(), dist.get_rank()
    order = np.random.default_rng(srand).permutation(rows).astype(np.int32)
    for at in range(0, rows, minibatch_size):
        batch = order[at:at + minibatch_size]
        lo, hi = shard(len(batch), world, rank)
        frames = batch[lo:hi]
        labels = (np.arange(hi - lo, dtype=np.int32), pdfs[frames], np.ones(hi - lo, np.float32))
        dp_xent_step_frames(net, corpus, frames, labels, grads, dist, len(batch), lo)
    return dp_objf_total(net, dist, reset=True)
