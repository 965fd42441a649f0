"""Training whole networks from labels under data parallelism, on the GPU:
the dropout mask by global row (DropoutComponent's row offset), the
cross-entropy derivative on its own (Nnet.XentDeriv), and kcnn_dp's
dp_xent_step / dp_train_epoch / dp_compute_prob_frames on two gloo ranks that
share the one GPU of the test box (RCCL needs a GPU per rank) against one
process on the whole minibatches.

The masks are Philox draws of (seed, call, GLOBAL row, column), so with equal
seeds the two ranks' shards carry exactly the masks of the single process, and
what is left between the two runs is rounding: the order of the shards' sums
and the f16x3 GEMMs' scale groups.  BAR is the bar tests/test_gpu_dp.py holds
the bench stacks to; profiles/dp_xent.md records what this network measures.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import nnet2_loss_ref as R
from _util import dev, host, rng

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
SEED = R.DROPOUT_SEED
BAR = 1e-5  # relative to the parameter's max-norm (tests/test_gpu_dp.py)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def assert_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = bits(a) != bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ in bits"


# ---- 1. the row offset ------------------------------------------------------------------
def mask_at(offset, call, rows, cols, dp=0.5, scale=0.0):
    """The mask of rows offset .. offset + rows - 1: Philox4x32-10 with key =
    the seed and counter (col // 4, offset + r, call low, call high)."""
    ncb = (cols + 3) // 4
    cb, row = np.meshgrid(np.arange(ncb, dtype=np.int64),
                          np.arange(rows, dtype=np.int64) + offset)
    assert row.max() < 1 << 32
    out = R.philox4x32_10(cb, row, call & 0xFFFFFFFF, call >> 32, SEED & 0xFFFFFFFF, SEED >> 32)
    x = np.stack(out, axis=-1).reshape(rows, ncb * 4)[:, :cols]
    u = (x >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    return R.dropout_mask(u, dp, scale)


def dropout(kc, dim, scale=0.0):
    c = kc.Component.NewFromString(
        f"DropoutComponent dim={dim} dropout-proportion=0.5 dropout-scale={scale}")
    c.SetDropoutSeed(SEED)
    return c


@pytest.mark.parametrize("dim", [24, 7])  # 16-byte accesses; the scalar kernel and its tail
def test_row_offset_bit_for_bit(kc, dim):
    import torch
    x = rng(dim).standard_normal((8, dim)).astype(F32)
    c = dropout(kc, dim)
    for offset in (0, 3, (1 << 31) + 5, (1 << 32) - 5):
        c.SetDropoutRowOffset(offset)
        c.SetDropoutSeed(SEED)  # restarts the call count
        for call in (0, 1):
            y = host(c.Propagate(dev(x[:5])))
            assert_bits(y, mask_at(offset, call, 5, dim) * x[:5], f"offset {offset} call {call}")
    # offset 0 is what there was before the offset: the reference's own generator
    assert_bits(mask_at(0, 1, 5, dim) * x[:5], R.dropout_prop(x[:5], 0.5, 0.0, SEED, 1), "ref")
    # offset 3 on 5 rows = rows 3 .. 7 of offset 0 on 8 rows, same seed and call
    whole, part = dropout(kc, dim), dropout(kc, dim)
    part.SetDropoutRowOffset(3)
    assert_bits(host(part.Propagate(dev(x[3:]))), host(whole.Propagate(dev(x)))[3:], "rows 3..7")
    # offset + rows > 2^32: an error, and nothing is written
    c.SetDropoutRowOffset((1 << 32) - 4)
    out = torch.full((5, dim), -7.0, device="cuda")
    with pytest.raises(kc.KcnnError, match="2\\^32"):
        c.Propagate(dev(x[:5]), out=out)
    torch.cuda.synchronize()
    assert (host(out) == -7.0).all()
    c.SetDropoutRowOffset((1 << 32) - 5)  # the same rows fit one lower
    c.Propagate(dev(x[:5]), out=out)
    assert not (host(out) == -7.0).any()
    # a copy starts at offset 0
    copy = c.Copy()
    copy.SetDropoutSeed(SEED)
    assert_bits(host(copy.Propagate(dev(x[:5]))), mask_at(0, 0, 5, dim) * x[:5], "Copy()")
    # high == low: no draw, whatever the offset
    flat = dropout(kc, dim, scale=1.0)
    flat.SetDropoutRowOffset(3)
    assert_bits(host(flat.Propagate(dev(x[:5]))), x[:5], "flat")
    with pytest.raises(kc.KcnnError, match="not a DropoutComponent"):
        kc.Component.NewFromString("SoftmaxComponent dim=4").SetDropoutRowOffset(1)


def test_nnet_set_row_offset(kc):
    """Every DropoutComponent of the stack; nothing for a stack without one;
    it holds until set again."""
    x = rng(5).standard_normal((5, 24)).astype(F32)
    net = kc.Nnet("DropoutComponent dim=24 dropout-proportion=0.5\n"
                  "DropoutComponent dim=24 dropout-proportion=0.5")
    net.SetRowOffset(3)
    for call in (0, 1):
        for c in net.components:
            c.SetDropoutSeed(SEED)
        m = mask_at(3, 0, 5, 24)
        net.Propagate(dev(x))
        assert_bits(host(net.Output()), m * (m * x), f"call {call}")
    kc.Nnet("SoftmaxComponent dim=4").SetRowOffset(3)


# ---- 2. XentDeriv + the generic backward = BackpropXent ---------------------------------
FC = ("FullyConnectedComponent input-dim={i} output-dim={o} learning-rate=0.02 "
      "param-stddev=0.2 bias-stddev=0.5 weight-decay=0.0005 momentum=0.9")
SOFTMAX_LAST = "\n".join([FC.format(i=20, o=32), "RectifiedLinearComponent dim=32",
                          "DropoutComponent dim=32 dropout-proportion=0.5",
                          FC.format(i=32, o=9), "SoftmaxComponent dim=9"])
# positive outputs from a last component that is not a Softmax
RELU_LAST = "\n".join([FC.format(i=20, o=9), "SoftmaxComponent dim=9",
                       "RectifiedLinearComponent dim=9"])


@pytest.mark.parametrize("config,literal", [(SOFTMAX_LAST, False), (SOFTMAX_LAST, True),
                                            (RELU_LAST, False)])
def test_xent_deriv_then_backward_is_backprop_xent(kc, config, literal):
    N = 37
    kc.set_randn_seed(31)
    base = kc.Nnet(config)
    nc = base.NumComponents()
    r = rng(32)
    x = dev(r.standard_normal((N, 20)).astype(F32))
    labels = [(n, int(r.integers(0, 9)), 1.0 if n % 3 else 0.5) for n in range(N) if n % 5]
    whole, halves = base.Copy(), base.Copy()
    for net in (whole, halves):
        for c in net.components:
            if c.Type() == "DropoutComponent":
                c.SetDropoutSeed(SEED)
    fused = config is SOFTMAX_LAST and not literal
    try:
        kc.set_literal_path(literal)
        whole.Propagate(x)
        whole.BackpropXent(labels)
        halves.Propagate(x)
        first, out_deriv = halves.XentDeriv(labels)
        assert first == (nc - 2 if fused else nc - 1)
        if fused:
            assert out_deriv is None
            # the last component's out_deriv was never formed: an error, not a stale read
            with pytest.raises(kc.KcnnError, match="kcnn_nnet_xent_deriv"):
                halves.BackpropComponent(nc - 1, None, mode=0, skip_first_dx=False)
        else:
            assert tuple(out_deriv.shape) == (N, 9)
        for i in reversed(range(first + 1)):
            halves.BackpropComponent(i, out_deriv, mode=0, skip_first_dx=False)
    finally:
        kc.set_literal_path(False)
    assert whole.ObjfTotal() == halves.ObjfTotal()
    assert whole.ObjfTotal()[1] == sum(w for _, _, w in labels)
    changed = False
    for i, (a, b, c0) in enumerate(zip(whole.components, halves.components, base.components)):
        if a.NumGradientParams() == 0:
            continue
        for which in (0, 1, 2):
            assert_bits(host(a.GetParam(which)), host(b.GetParam(which)),
                        f"component {i} parameter {which}")
        changed |= not np.array_equal(host(a.GetParam(0)), host(c0.GetParam(0)))
    assert changed
    assert_bits(host(whole.InputDeriv(0)), host(halves.InputDeriv(0)), "InputDeriv(0)")


# ---- 3, 4. two ranks against one process ------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_worker(tmp_path, what, split, backend, nproc):
    """One launch with a time limit of its own; never retried."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr=127.0.0.1",
           f"--master-port={_free_port()}", os.path.join(HERE, "dp_xent_gpu_worker.py"),
           str(tmp_path), what, backend]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    if split:
        env["KCNN_DP_SPLIT_PARAMS"] = split
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return (np.load(tmp_path / "rank0.npz"), np.load(tmp_path / f"rank{nproc - 1}.npz"),
            np.load(tmp_path / "single.npz"))


def check_replicas(a, b, single, what):
    """Replicas bitwise identical; against the single process every parameter
    and momentum buffer within BAR of its max-norm."""
    assert sorted(a.files) == sorted(single.files)
    names = [k for k in a.files if k[0] in "Wbp" and k[1:].isdigit()]
    assert len(names) == 9  # conv and two FC: weights, bias, momentum buffer
    worst = 0.0
    for k in names:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"replicas differ: {k}")
        ref = single[k]
        err = np.abs(a[k] - ref).max() / max(np.abs(ref).max(), 1e-30)
        print(f"{what} {k}: DP vs single-process relative error {err:.3e}")
        worst = max(worst, err)
    print(f"{what}: worst {worst:.3e} (bar {BAR:.1e})")
    return worst


def check_totals(a, b, single, key, exact, what):
    np.testing.assert_array_equal(a[key], b[key])   # all-reduced: the same on every rank
    got, want = a[key], single[key]
    rel = abs(got[0] - want[0]) / abs(want[0])
    print(f"{what} {key}: {got.tolist()} vs {want.tolist()} (objective rel {rel:.3e})")
    for k in exact:
        assert got[k] == want[k], f"{what} {key}[{k}]: {got[k]} vs {want[k]}"
    assert want[0] < 0 and rel < BAR, f"{what} {key}: objective relative error {rel:.2e}"


@pytest.mark.parametrize("split,backend,nproc", [(None, "gloo", 2), ("1", "gloo", 2),
                                                 (None, "nccl", 1)])
def test_dp_xent_steps_match_single_process(tmp_path, split, backend, nproc):
    """Two steps, n_global = 48 and 37 (shards of 18 / 19).  split "1": every
    affine gradient on its own all-reduce, started before the layer's data
    gradient.  nccl: the RCCL communicator at world size 1."""
    a, b, single = run_worker(tmp_path, "steps", split, backend, nproc)
    what = f"steps split={split} {backend}"
    worst = check_replicas(a, b, single, what)
    check_totals(a, b, single, "objf", exact=(1,), what=what)
    assert single["objf"][1] == 16 * 0.5 + 32 + 13 * 0.5 + 24  # the weight, not the 85 rows
    assert worst < BAR, f"{what}: worst relative error {worst:.2e}"


def test_dp_train_epoch_matches_train_epoch(tmp_path):
    """49 corpus rows in minibatches of 16 on two ranks: the last minibatch
    has one row and leaves rank 0's shard empty.  Then evaluation of 37
    held-out rows (dp_compute_prob_frames), the Dropout drawing its masks."""
    a, b, single = run_worker(tmp_path, "epoch", None, "gloo", 2)
    worst = check_replicas(a, b, single, "epoch")
    check_totals(a, b, single, "objf", exact=(1,), what="epoch")
    assert single["objf"][1] == 49
    check_totals(a, b, single, "prob", exact=(1, 2), what="held-out")
    assert single["prob"][1] == 10 * 0.25 + 27
    assert worst < BAR, f"epoch: worst relative error {worst:.2e}"
