"""Data-parallel training from labels (kaldi-cnn_amd/kcnn_dp.py) on the CPU:
shard() partitions a minibatch, and two gloo ranks running dp_xent_step on a
numpy stand-in (FC -> Softmax in fp64, from tests/nnet2_loss_ref.py) end with
identical replicas that match one process on the whole batch -- also when the
global minibatch has one row, so that one rank's shard is empty: that rank
runs no forward pass, joins the same collectives over zeroed gradients and
applies the same update.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as tdist
import torch.multiprocessing as mp

import kcnn_dp
import nnet2_loss_ref as R

IN, OUT, LR = 7, 5, 0.05


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 2, 37, 48])
def test_shard_partitions_the_minibatch(n, world):
    pieces = [kcnn_dp.shard(n, world, r) for r in range(world)]
    assert pieces[0][0] == 0 and pieces[-1][1] == n
    for (lo, hi), (lo2, _) in zip(pieces, pieces[1:]):
        assert hi == lo2                                   # contiguous and disjoint
    sizes = [hi - lo for lo, hi in pieces]
    assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1 and sum(sizes) == n


class _FC:
    def __init__(self, r):
        self.W = r.standard_normal((OUT, IN)) * 0.3
        self.b = r.standard_normal(OUT) * 0.1

    def Type(self):
        return "FullyConnectedComponent"

    def NumGradientParams(self):
        return self.W.size + self.b.size

    def ApplyGradient(self, grad, n):
        g = grad.numpy()
        self.W = self.W + LR / n * g[:self.W.size].reshape(self.W.shape)
        self.b = self.b + LR / n * g[self.W.size:]


class _Softmax:
    def Type(self):
        return "SoftmaxComponent"

    def NumGradientParams(self):
        return 0


class NumpyNet:
    """kcnn.Nnet's host interface, as kcnn_dp uses it, over an fp64 FC ->
    Softmax: XentDeriv takes the fused route (first = nc - 2, no out_deriv)."""

    def __init__(self, seed):
        self.components = [_FC(np.random.default_rng(seed)), _Softmax()]
        self.offsets, self.forwards, self.objf = [], 0, np.zeros(2)

    def NumComponents(self):
        return 2

    def SetRowOffset(self, offset):
        self.offsets.append(offset)

    def Propagate(self, x):
        fc = self.components[0]
        self.x = x.numpy()
        assert self.x.shape[0] > 0, "a forward pass on an empty shard"
        self.p = R.softmax_prop64(self.x @ fc.W.T + fc.b)
        self.forwards += 1

    def XentDeriv(self, labels):
        triples = [(int(r), int(c), float(w)) for r, c, w in zip(*labels)]
        self.deriv, _ = R.xent_deriv64(self.p, triples)
        for r, c, w in triples:
            self.objf += (w * np.log(self.p[r, c]), w)
        return 0, None

    def BackpropComponent(self, i, out_deriv, mode, grad=None, skip_first_dx=True):
        assert i == 0 and out_deriv is None
        if mode in (1, 3):
            g = np.concatenate([(self.deriv.T @ self.x).ravel(), self.deriv.sum(axis=0)])
            grad.copy_(torch.from_numpy(g))

    def BackpropSplit(self, i, out_deriv, grad, skip_first_dx, between):
        self.BackpropComponent(i, out_deriv, 3, grad, skip_first_dx)
        between()
        self.BackpropComponent(i, out_deriv, 2, None, skip_first_dx)

    def ObjfTotal(self, reset=False):
        out = tuple(self.objf)
        if reset:
            self.objf = np.zeros(2)
        return out


def _batches(n_global):
    r = np.random.default_rng(100 + n_global)
    out = []
    for _ in range(2):
        x = r.standard_normal((n_global, IN))
        cols = r.integers(0, OUT, size=n_global).astype(np.int32)
        out.append((x, cols))
    return out


def _step(net, grads, dist, x, cols, lo, hi):
    n = hi - lo
    labels = (np.arange(n, dtype=np.int32), cols[lo:hi], np.ones(n, np.float32))
    kcnn_dp.dp_xent_step(net, torch.from_numpy(x[lo:hi]), labels, grads, dist, len(x), lo)


def _alloc(n):
    return torch.empty(n, dtype=torch.float64)


def _params(net):
    return np.concatenate([net.components[0].W.ravel(), net.components[0].b])


def _worker(rank, world, port, q, split, n_global):
    kcnn_dp.SPLIT_GRADIENT_PARAMS = split
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    net = NumpyNet(seed=5)                               # identical replicas
    grads = kcnn_dp.gradient_buffers(net, _alloc)
    for x, cols in _batches(n_global):
        _step(net, grads, tdist, x, cols, *kcnn_dp.shard(n_global, world, rank))
    total = kcnn_dp.dp_objf_total(net, tdist, reset=True)
    q.put((rank, (_params(net), net.forwards, net.offsets, total)))
    tdist.barrier()
    tdist.destroy_process_group()


class _LocalDist:
    """world_size 1: the all-reduce is the identity."""
    class _W:
        def wait(self):
            pass

    def all_reduce(self, t, async_op=False):
        return self._W()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("n_global,split", [(1, 1 << 20), (5, 1 << 20), (1, 1), (5, 1)])
def test_two_ranks_xent_step_equals_one_process(n_global, split, monkeypatch):
    """n_global = 1: rank 0's shard [0, 0) is empty.  split = 1: the FC
    gradient on its own all-reduce (BackpropSplit), else in the flat bucket."""
    monkeypatch.setattr(kcnn_dp, "SPLIT_GRADIENT_PARAMS", split)
    ref = NumpyNet(seed=5)
    grads = kcnn_dp.gradient_buffers(ref, _alloc)
    for x, cols in _batches(n_global):
        _step(ref, grads, _LocalDist(), x, cols, 0, n_global)
    want, want_total = _params(ref), ref.ObjfTotal()

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, split, n_global))
             for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0                            # both ranks finish
    np.testing.assert_array_equal(got[0][0], got[1][0])   # replicas stay identical
    assert not np.array_equal(want, _params(NumpyNet(seed=5)))  # and something was learnt
    for r in range(2):
        # fp64 throughout: only the order of the two shards' sums differs
        np.testing.assert_allclose(got[r][0], want, rtol=1e-12, atol=1e-14)
        lo, hi = kcnn_dp.shard(n_global, 2, r)
        assert got[r][1] == (2 if hi > lo else 0)         # no forward on an empty shard
        assert got[r][2] == ([lo, lo] if hi > lo else [])
        assert got[r][3][1] == want_total[1] == 2 * n_global
        np.testing.assert_allclose(got[r][3][0], want_total[0], rtol=1e-12)
