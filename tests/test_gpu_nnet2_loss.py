"""SoftmaxComponent, DropoutComponent and the cross-entropy training step on
the GPU against the numpy restatement of tests/nnet2_loss_ref.py.

Bars: the project's 1e-5 bound against fp64 for everything that rounds
(softmax outputs: rtol 1e-5 after the floor; derivatives: 1e-5 * the sum of
|terms|; parameters: 1e-5 normwise); bit-exact where the fp32 operation
sequence is fixed (CompObjfAndDeriv's derivative, Dropout both ways, model
files).

The *_layouts tests call the kn_* launchers directly on pitched operands with
sentinels, at the shapes and layouts of tests/nnet2_kernel_cases.py: every
access width (4, 2, 1 columns a lane) at every count of values a lane holds,
either side of each step (256 | 257, 1024 | 1025, 4096 | 4097), 1 and 70 rows;
tests/test_nnet2_routes.py pins the kernel each case launches.  Same
references, same bars."""
import os

import numpy as np
import pytest

import nnet2_kernel_cases as T
import nnet2_loss_ref as R
from _pitched import GUARD, PAD, assert_bits, edge_columns, place, stream, sync
from _util import assert_same, dev, host, padded, rng

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = os.path.join(GOLDEN, "models")
DROPOUT_SEED = R.DROPOUT_SEED
COLS = [1, 2, 63, 64, 65, 1000, 3454, 4096, 4097]
FLOOR = np.float32(1.0e-20)
F32 = np.float32


def softmax_input(rows, cols, seed=0):
    """N(0, 1) * 4; the first row holds one -inf (when it has another
    element); with 70 rows, rows 1 and 2 hold entries +-80 and +-1e4."""
    x = (rng(seed).standard_normal((rows, cols)) * 4).astype(F32)
    if cols > 1:
        x[0, cols // 2] = -np.inf
    if rows > 2:
        x[1, ::3], x[1, 1::3] = 80.0, -80.0
        x[2, ::5], x[2, 2::5] = 1.0e4, -1.0e4
    return x


def check_softmax(y, x):
    raw = R.softmax_raw64(x)
    t = R.softmax_prop64(x)
    y64 = y.astype(np.float64)
    rel = np.abs(y64 - t) / t
    print(f"softmax {x.shape}: worst rel err {rel.max():.3e}, "
          f"worst row-sum err {np.abs(y64.sum(axis=1) - 1).max():.3e}")
    assert (rel <= 1e-5).all(), f"{(rel > 1e-5).sum()} elements past rtol 1e-5, worst {rel.max():.3e}"
    assert (np.abs(y64.sum(axis=1) - 1) <= 1e-5).all()
    assert (y[raw < 0.5e-20] == FLOOR).all()
    if x.shape[1] > 1:
        assert y[0, x.shape[1] // 2] == FLOOR  # the -inf


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", [1, 70])
def test_softmax_propagate(kc, rows, cols):
    x = softmax_input(rows, cols)
    c = kc.Component.NewFromString(f"SoftmaxComponent dim={cols}")
    assert c.Type() == "SoftmaxComponent" and c.InputDim() == c.OutputDim() == cols
    assert not c.BackpropNeedsInput() and c.BackpropNeedsOutput()
    check_softmax(host(c.Propagate(dev(x))), x)


@pytest.mark.parametrize("extra", [0, 2])
def test_softmax_propagate_3454_strides(kc, extra):
    """3454 columns at row stride 3456 (16-byte rows) and 3454 (odd rows only
    8-byte aligned); the pad columns of the output stay untouched."""
    import torch
    x = softmax_input(70, 3454, seed=1)
    c = kc.Component.NewFromString("SoftmaxComponent dim=3454")
    xd = padded(x, extra) if extra else dev(x)
    base = torch.full((70, 3454 + extra), float("nan"), dtype=torch.float32, device="cuda")
    out = base[:, :3454]
    assert xd.stride(0) == out.stride(0) == 3454 + extra
    c.Propagate(xd, out=out)
    check_softmax(host(out), x)
    assert torch.isnan(base[:, 3454:]).all()


def test_softmax_propagate_inf_row(kc):
    x = softmax_input(70, 1000, seed=2)
    c = kc.Component.NewFromString("SoftmaxComponent dim=1000")
    clean = host(c.Propagate(dev(x)))
    x2 = x.copy()
    x2[3, 17] = np.inf
    y = host(c.Propagate(dev(x2)))
    assert np.isnan(y[3]).all()
    keep = np.arange(70) != 3
    assert (y[keep].view(np.int32) == clean[keep].view(np.int32)).all()


@pytest.mark.parametrize("cols", COLS)
def test_softmax_backprop_general(kc, cols):
    r = rng(cols)
    p = R.softmax_prop64(r.standard_normal((70, cols)) * 2).astype(F32)
    e = r.standard_normal((70, cols)).astype(F32)
    c = kc.Component.NewFromString(f"SoftmaxComponent dim={cols}")
    pd, ed = dev(p), dev(e)
    t, s = R.softmax_backprop64(p, e)
    for update in (False, True, True):
        d = host(c.Backprop(None, pd, ed, update=update)).astype(np.float64)
        err = np.abs(d - t) / np.maximum(s, 1e-300)
        print(f"softmax backprop cols={cols}: worst err / sum|P E| = {err.max():.3e}")
        assert (np.abs(d - t) <= 1e-5 * s).all(), err.max()
    vs, ds, cnt = c.NonlinearStats()
    assert cnt == 140
    assert ds.size == 0 or not ds.any()
    np.testing.assert_allclose(vs, 2 * p.astype(np.float64).sum(axis=0), rtol=2e-6, atol=1e-5)


def hard_labels(r, rows, cols):
    return [(i, int(r.integers(cols)), 1.0) for i in range(rows)]


def soft_labels(r, rows, cols, skip=()):
    """1 to 3 labels a row with weights k / 8, sorted by row, none repeated."""
    out = []
    for i in range(rows):
        if i in skip:
            continue
        k = min(int(r.integers(1, 4)), cols)
        for c in sorted(r.choice(cols, size=k, replace=False)):
            out.append((i, int(c), float(r.integers(1, 9)) / 8))
    return out


@pytest.mark.parametrize("soft", [False, True])
def test_comp_objf_and_deriv(kc, soft):
    r = rng(5)
    p = R.softmax_prop64(r.standard_normal((70, 65)) * 3).astype(F32)
    start = r.standard_normal((70, 65)).astype(F32)
    labels = soft_labels(r, 70, 65) if soft else hard_labels(r, 70, 65)
    exp_d, exp_objf, exp_w = R.comp_objf_and_deriv32(p, labels, start)
    got = []
    for _ in range(2):
        d = dev(start)
        objf, w = kc.comp_objf_and_deriv(dev(p), labels, d)
        got.append((host(d), objf, w))
    assert_same(got[0][0], exp_d, "deriv += w / p")
    assert got[0][2] == exp_w
    print(f"objf {got[0][1]!r} vs fp64 {exp_objf!r}")
    assert abs(got[0][1] - exp_objf) <= 1e-6 * abs(exp_objf)
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2]
    assert (got[0][0].view(np.int32) == got[1][0].view(np.int32)).all()
    with pytest.raises(kc.KcnnError, match="repeated"):
        kc.comp_objf_and_deriv(dev(p), labels + [labels[3]], dev(start))
    with pytest.raises(kc.KcnnError, match="outside"):
        kc.comp_objf_and_deriv(dev(p), [(70, 0, 1.0)], dev(start))


FC = ("FullyConnectedComponent input-dim={i} output-dim={o} learning-rate=0.02 "
      "param-stddev={s} bias-stddev=0.5 weight-decay=0.0005 momentum=0.9")


def fc_params(kc, c):
    return [host(c.GetParam(w)).astype(np.float64)
            for w in (kc.PARAM_LINEAR, kc.PARAM_BIAS, kc.PARAM_PREV_GRAD)]


def fc64(kc, c):
    W, b, prev = fc_params(kc, c)
    return R.FC64(W, b.ravel(), prev, float(F32(0.02)), float(F32(0.0005)), float(F32(0.9)))


def normwise(a, t):
    a, t = np.asarray(a, np.float64).ravel(), np.asarray(t, np.float64).ravel()
    return np.linalg.norm(a - t) / max(np.linalg.norm(t), 1e-300)


def xent_step(kc, config, x, labels, literal):
    """A fresh stack (same parameters every time), one Propagate, then
    BackpropXent on the fused or the literal path; returns what the
    comparison needs."""
    kc.set_randn_seed(77)
    net = kc.Nnet(config)
    fc, sm = net.components[-2], net.components[-1]
    before = fc64(kc, fc)
    net.Propagate(x)
    p = host(net.Output())
    kc.set_literal_path(literal)
    try:
        net.BackpropXent(labels)
        d = host(net.InputDeriv(net.NumComponents() - 1))
    finally:
        kc.set_literal_path(False)
    return dict(before=before, p=p, d=d, params=fc_params(kc, fc), objf=net.ObjfTotal(),
                stats=sm.NonlinearStats())


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("dim,rows", [(10, 37), (3454, 5)])
def test_fused_against_literal(kc, dim, rows, soft):
    config = FC.format(i=24, o=dim, s=0.3) + f"\nSoftmaxComponent dim={dim}"
    r = rng(dim + soft)
    xh = r.standard_normal((rows, 24)).astype(F32)
    x = dev(xh)
    labels = soft_labels(r, rows, dim, skip=(2,)) if soft else hard_labels(r, rows, dim)
    fused = xent_step(kc, config, x, labels, literal=False)
    lit = xent_step(kc, config, x, labels, literal=True)
    assert_same(fused["p"], lit["p"], "softmax output")
    p = fused["p"]
    # the fp64 restatement from the stack's own softmax output
    t, s = R.xent_deriv64(p, labels)
    for name, got in (("fused", fused), ("literal", lit)):
        err = np.abs(got["d"].astype(np.float64) - t)
        print(f"{name} dim={dim} soft={soft}: worst |D - D64| / S_r = "
              f"{(err / np.maximum(s, 1e-300)).max():.3e}")
        assert (err <= 1e-5 * s).all(), name
    ref = fused["before"]
    ref.backprop(xh.astype(np.float64), t)
    for k, (a, b, c) in enumerate(zip(fused["params"], lit["params"],
                                      (ref.W, ref.b, ref.prev))):
        print(f"param {k}: fused/literal {normwise(a, b):.2e}, fused/fp64 {normwise(a, c):.2e}, "
              f"literal/fp64 {normwise(b, c):.2e}")
        assert normwise(a, b) <= 1e-5 and normwise(a, c) <= 1e-5 and normwise(b, c) <= 1e-5
    objf64 = sum(float(F32(w)) * np.log(np.float64(p[i, c])) for i, c, w in labels)
    wsum = sum(float(F32(w)) for _, _, w in labels)
    for got in (fused, lit):
        assert abs(got["objf"][0] - objf64) <= 1e-6 * abs(objf64)
        assert got["objf"][1] == wsum
        vs, ds, cnt = got["stats"]
        assert cnt == rows and (ds.size == 0 or not ds.any())
        np.testing.assert_allclose(vs, p.astype(np.float64).sum(axis=0), rtol=2e-6, atol=1e-5)
    assert abs(fused["objf"][0] - lit["objf"][0]) <= 1e-6 * abs(objf64)


@pytest.mark.parametrize("literal", [False, True])
def test_label_validation(kc, literal):
    config = FC.format(i=24, o=10, s=0.3) + "\nSoftmaxComponent dim=10"
    kc.set_randn_seed(78)
    net = kc.Nnet(config)
    fc = net.components[0]
    x = dev(rng(9).standard_normal((37, 24)).astype(F32))
    good = hard_labels(rng(10), 37, 10)
    kc.set_literal_path(literal)
    try:
        net.Propagate(x)
        before = fc_params(kc, fc)
        bad = {"outside": [good[:5] + [(37, 0, 1.0)], good[:5] + [(-1, 0, 1.0)],
                           good[:5] + [(5, 10, 1.0)], [(0, -1, 1.0)]],
               "not sorted": [[good[4], good[3]]],
               "repeated": [[good[3], good[3]], [(3, 1, 0.5), (3, 2, 0.25), (3, 1, 0.25)]]}
        for what, cases in bad.items():
            for labels in cases:
                with pytest.raises(kc.KcnnError, match=what):
                    net.BackpropXent(labels)
        # nothing ran: no objective, no update
        assert net.ObjfTotal() == (0.0, 0.0)
        for a, b in zip(before, fc_params(kc, fc)):
            assert_same(a, b, "parameters after refused labels")
        net.BackpropXent(good)
        objf, w = net.ObjfTotal()
        assert w == 37 and np.isfinite(objf) and objf < 0
        assert any((a != b).any() for a, b in zip(before, fc_params(kc, fc)))
    finally:
        kc.set_literal_path(False)


def relu_like(r, shape):
    x = r.standard_normal(shape).astype(F32)
    return np.where(x < 0, F32(0), x)


@pytest.mark.parametrize("dp,scale", [(0.5, 0.0), (0.2, 0.5), (0.0, 0.0), (0.5, 1.0)])
@pytest.mark.parametrize("dim", [4095, 4096])
def test_dropout(kc, dim, dp, scale):
    line = f"DropoutComponent dim={dim} dropout-proportion={dp} dropout-scale={scale}"
    c = kc.Component.NewFromString(line)
    assert c.Type() == "DropoutComponent" and c.InputDim() == c.OutputDim() == dim
    assert c.BackpropNeedsInput() and c.BackpropNeedsOutput()
    c.SetDropoutSeed(DROPOUT_SEED)
    assert c.DropoutSeed() == DROPOUT_SEED
    r = rng(dim)
    x = relu_like(r, (70, dim))
    xd = dev(x)
    outs = [host(c.Propagate(xd)) for _ in range(3)]
    for k, y in enumerate(outs):
        assert_same(y, R.dropout_prop(x, dp, scale, DROPOUT_SEED, k), f"call {k}")
    if (dp, scale) in ((0.5, 1.0), (0.0, 0.0)):
        for y in outs:
            assert (y.view(np.int32) == x.view(np.int32)).all()
    elif scale == 0.0:
        assert not (outs[0] == outs[1]).all()
    other = kc.Component.NewFromString(line)
    other.SetDropoutSeed(DROPOUT_SEED)
    assert_same(host(other.Propagate(xd)), outs[0], "same seed, another component")
    # Backprop: AddMatMatDivMat on an input with exact zeros and an inf derivative
    od = r.standard_normal((70, dim)).astype(F32)
    zero, nonzero = np.argwhere(x == 0)[0], np.argwhere(x != 0)[:2]
    od[tuple(zero)] = np.inf
    od[tuple(nonzero[0])] = np.inf
    od[tuple(nonzero[1])] = -np.inf
    dx = c.Backprop(xd, dev(outs[2]), dev(od))
    assert_same(host(dx), R.dropout_backprop(x, outs[2], od), "Backprop")


@pytest.mark.parametrize("line", ["DropoutComponent dim=8 dropout-proportion=1.0",
                                  "DropoutComponent dim=8 dropout-scale=1.5"])
def test_dropout_asserts(kc, line):
    c = kc.Component.NewFromString(line)
    with pytest.raises(kc.KcnnError):
        c.Propagate(dev(np.ones((2, 8), F32)))


def test_dropout_init_from_string(kc):
    c = kc.Component.NewFromString("DropoutComponent dim=8")
    assert c.Info().endswith("dropout_proportion = 0.5, dropout_scale = 0")
    with pytest.raises(kc.KcnnError):
        kc.Component.NewFromString("DropoutComponent dim=8 dropout-rate=0.1")
    with pytest.raises(kc.KcnnError):
        kc.Component.NewFromString("DropoutComponent dropout-proportion=0.1")
    # scale 1.0 is inference: the identity
    c.SetDropoutScale(1.0)
    x = rng(3).standard_normal((5, 8)).astype(F32)
    assert_same(host(c.Propagate(dev(x))), x)
    # the seed comes from the host generator
    seeds = []
    for _ in range(2):
        kc.set_randn_seed(1234)
        seeds.append(kc.Component.NewFromString("DropoutComponent dim=8").DropoutSeed())
    assert seeds[0] == seeds[1]
    assert kc.Component.NewFromString("DropoutComponent dim=8").DropoutSeed() != seeds[0]


@pytest.mark.parametrize("kind", ["dropout", "softmax"])
def test_model_io(kc, tmp_path, kind):
    path = os.path.join(MODELS, f"{kind}.bin")
    z = np.load(os.path.join(MODELS, f"{kind}.npz"))
    c = kc.Component.ReadNew(path)
    assert c.Type() == {"dropout": "DropoutComponent", "softmax": "SoftmaxComponent"}[kind]
    assert c.InputDim() == int(z["dim"])
    if kind == "softmax":
        vs, ds, cnt = c.NonlinearStats()
        np.testing.assert_array_equal(vs, z["value_sum"])
        np.testing.assert_array_equal(ds, z["deriv_sum"])
        assert cnt == float(z["count"])
    else:
        assert c.Info().endswith("dropout_proportion = 0.375, dropout_scale = 0.25")
    out = tmp_path / f"{kind}.bin"
    c.Write(out, True)
    assert open(out, "rb").read() == open(path, "rb").read()
    text = tmp_path / f"{kind}.txt"
    c.Write(text, False)
    assert kc.Component.ReadNew(text).Info() == c.Info()
    copy = c.Copy()
    assert copy.Info() == c.Info()
    if kind == "dropout":
        assert copy.DropoutSeed() != c.DropoutSeed()


def test_reference_nnet_config_trains_a_step(kc):
    """The reference's own model file, whole.  Its last FC starts at zero, so
    the first step's answer is known: every output 1 / 3454, the objective
    -ln 3454 a frame, the derivative into the Softmax onehot - 1 / 3454; only
    that FC receives a gradient in step 1 (every derivative below it is a
    product with its zero weights), so step 2 scores the same minibatch
    strictly higher.  Dropout scale 1 (inference) makes it deterministic."""
    kc.set_randn_seed(2026)
    net = kc.Nnet(open(os.path.join(GOLDEN, "nnet.config")).read())
    assert net.NumComponents() == 22
    assert [c.Type() for c in net.components][-3:] == [
        "DropoutComponent", "FullyConnectedComponent", "SoftmaxComponent"]
    for c in net.components:
        if c.Type() == "DropoutComponent":
            c.SetDropoutScale(1.0)
    r = rng(11)
    x = dev(r.standard_normal((8 * 21, 40)).astype(F32))
    labels = hard_labels(r, 8, 3454)
    net.Propagate(x)
    p = host(net.Output())
    assert p.shape == (8, 3454)
    # fp32 1 / 3454 from exp(0) / 3454: within an ulp; the issue's bar is 1e-6
    np.testing.assert_allclose(p, 1.0 / 3454, rtol=1e-6)
    net.BackpropXent(labels)
    objf, w = net.ObjfTotal(reset=True)
    assert w == 8 and abs(objf - (-8 * np.log(3454.0))) <= 1e-6 * 8 * np.log(3454.0)
    onehot = np.zeros((8, 3454))
    for i, c, _ in labels:
        onehot[i, c] = 1.0
    # D = onehot - P with P within 1e-6 of 1 / 3454 and one fp32 rounding
    np.testing.assert_allclose(host(net.InputDeriv(21)), onehot - 1.0 / 3454, rtol=2e-6)
    net.Propagate(x)
    net.BackpropXent(labels)
    objf2, w2 = net.ObjfTotal()
    assert w2 == 8 and objf2 / w2 > objf / w


def test_small_end_to_end(kc):
    """FC -> ReLU -> Dropout -> FC -> Softmax, two steps from labels, against
    an fp64 chain whose masks come from the numpy Philox."""
    config = "\n".join([FC.format(i=24, o=32, s=0.3), "RectifiedLinearComponent dim=32",
                        "DropoutComponent dim=32 dropout-proportion=0.5 dropout-scale=0.0",
                        FC.format(i=32, o=10, s=0.3), "SoftmaxComponent dim=10"])
    kc.set_randn_seed(79)
    net = kc.Nnet(config)
    net.components[2].SetDropoutSeed(DROPOUT_SEED)
    f1, f2 = fc64(kc, net.components[0]), fc64(kc, net.components[3])
    r = rng(12)
    xh = r.standard_normal((37, 24)).astype(F32)
    x, x64 = dev(xh), xh.astype(np.float64)
    labels = soft_labels(r, 37, 10)
    objf64 = 0.0
    for step in range(2):
        net.Propagate(x)
        net.BackpropXent(labels)
        mask = R.dropout_mask(R.dropout_uniform(DROPOUT_SEED, step, 37, 32), 0.5, 0.0)
        h1 = np.maximum(f1.propagate(x64), 0.0)
        h2 = h1 * mask
        p = R.softmax_prop64(f2.propagate(h2))
        objf64 += sum(float(F32(w)) * np.log(p[i, c]) for i, c, w in labels)
        d, _ = R.xent_deriv64(p, labels)
        dh1 = f2.backprop(h2, d) * mask * (h1 > 0)
        f1.backprop(x64, dh1)
        for name, comp, ref in (("fc1", net.components[0], f1), ("fc2", net.components[3], f2)):
            for k, (a, t) in enumerate(zip(fc_params(kc, comp), (ref.W, ref.b, ref.prev))):
                print(f"step {step} {name} param {k}: normwise {normwise(a, t):.2e}")
                assert normwise(a, t) <= 1e-5, (step, name, k)
    objf, w = net.ObjfTotal()
    print(f"objf {objf!r} vs fp64 {objf64!r}")
    assert abs(objf - objf64) <= 1e-5 * abs(objf64)
    assert w == 2 * sum(float(F32(wt)) for _, _, wt in labels)


# ---- every (access width, values a lane) instantiation, through the launchers -------------
@pytest.fixture(scope="module")
def KN(kc):
    return T.bind(kc)


def edge_input(rows, cols, seed=0):
    """softmax_input with a -inf also in row 0's last column, in the last column
    of its last whole vector and in the first column of the element-wise tail."""
    x = softmax_input(rows, cols, seed)
    x[0, edge_columns(cols)] = -np.inf
    return x


def stats_buffers(KN, dim, cols):
    """value_sum (zero, then a NaN guard) and the workspace (then a PAD guard)."""
    import torch
    vs = torch.full((cols + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    vs[:cols] = 0
    n = KN.kn_softmax_stats_ws(dim) // 4
    ws = torch.full((n + GUARD,), float(PAD), dtype=torch.float32, device="cuda")
    return vs, ws, n


def check_stats_buffers(vs, ws, n, cols, want, what):
    got = vs.cpu().numpy()
    assert np.isnan(got[cols:]).all(), "words after value_sum were written"
    assert (ws[n:].cpu().numpy() == PAD).all(), "workspace guard was written"
    np.testing.assert_allclose(got[:cols], want, rtol=2e-6, atol=1e-5, err_msg=what)


@pytest.mark.parametrize("case", T.select("kn_softmax_prop"), ids=T.name_of)
def test_softmax_propagate_layouts(kc, KN, case):
    rows, cols = case["rows"], case["cols"]
    x = edge_input(rows, cols, seed=3)
    X, Y = place(kc, case["ops"][0], x), place(kc, case["ops"][1])
    assert KN.kn_softmax_prop(X.ptr, X.dim, Y.ptr, Y.dim, stream()) == 0
    sync()
    y = Y.get()
    check_softmax(y, x)
    assert (y[0, edge_columns(cols)] == FLOOR).all()
    assert_bits(X.get(), x, "the input")
    if rows == 1:
        # the only row's edge columns hold -inf: a dropped last column would not
        # show, so the same row with numbers there as well
        x = softmax_input(rows, cols, seed=3)
        X, Y = place(kc, case["ops"][0], x), place(kc, case["ops"][1])
        assert KN.kn_softmax_prop(X.ptr, X.dim, Y.ptr, Y.dim, stream()) == 0
        sync()
        check_softmax(Y.get(), x)


@pytest.mark.parametrize("case", T.select("kn_softmax_backprop"), ids=T.name_of)
def test_softmax_backprop_layouts(kc, KN, case):
    rows, cols = case["rows"], case["cols"]
    r = rng(cols + rows)
    p = R.softmax_prop64(r.standard_normal((rows, cols)) * 2).astype(F32)
    e = r.standard_normal((rows, cols)).astype(F32)
    Pm, Em, Dm = place(kc, case["ops"][0], p), place(kc, case["ops"][1], e), place(kc, case["ops"][2])
    vs, ws, n = stats_buffers(KN, Pm.dim, cols)
    t, s = R.softmax_backprop64(p, e)
    calls = 2 if case["stats"] else 1
    for _ in range(calls):
        assert KN.kn_softmax_backprop(Pm.ptr, Pm.dim, Em.ptr, Em.dim, Dm.ptr, Dm.dim,
                                      vs.data_ptr() if case["stats"] else None,
                                      ws.data_ptr() if case["stats"] else None, stream()) == 0
        sync()
        d = Dm.get().astype(np.float64)
        err = np.abs(d - t) / np.maximum(s, 1e-300)
        print(f"softmax backprop {case['name']}: worst err / sum|P E| = {err.max():.3e}")
        assert (np.abs(d - t) <= 1e-5 * s).all(), err.max()
    want = calls * p.astype(np.float64).sum(axis=0) if case["stats"] else np.zeros(cols)
    check_stats_buffers(vs, ws, n, cols, want, case["name"])
    assert_bits(Pm.get(), p, "out_value")
    assert_bits(Em.get(), e, "out_deriv")


def edge_labels(r, rows, cols, skip=()):
    """soft_labels, and in row 0 a label in each edge column as well."""
    labels = [l for l in soft_labels(r, rows, cols, skip) if l[0] != 0]
    return [(0, c, (k + 1) / 8) for k, c in enumerate(edge_columns(cols))] + labels


def label_arrays(labels, rows):
    import torch
    count = np.bincount([l[0] for l in labels], minlength=rows)
    row_start = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    col = np.array([l[1] for l in labels], np.int32)
    w = np.array([l[2] for l in labels], F32)
    return [torch.from_numpy(a).cuda() for a in (row_start, col, w)]


@pytest.mark.parametrize("case", T.select("kn_softmax_xent_backprop"), ids=T.name_of)
def test_softmax_xent_layouts(kc, KN, case):
    import torch
    rows, cols = case["rows"], case["cols"]
    r = rng(2 * cols + rows)
    p = R.softmax_prop64(r.standard_normal((rows, cols)) * 2).astype(F32)
    labels = edge_labels(r, rows, cols, skip=(2,))
    row_start, lab_col, lab_w = label_arrays(labels, rows)
    Pm, Dm = place(kc, case["ops"][0], p), place(kc, case["ops"][1])
    vs, ws, n = stats_buffers(KN, Pm.dim, cols)
    nb = KN.kn_softmax_xent_blocks(Pm.dim)
    objf_n = KN.kn_objf_ws(nb) // 8
    assert objf_n == 2 * nb
    objf_ws = torch.full((objf_n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    tot = torch.full((2 + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    tot[:2] = 0
    assert KN.kn_softmax_xent_backprop(Pm.ptr, Pm.dim, Dm.ptr, Dm.dim, row_start.data_ptr(),
                                       lab_col.data_ptr(), lab_w.data_ptr(),
                                       vs.data_ptr() if case["stats"] else None,
                                       ws.data_ptr() if case["stats"] else None, tot.data_ptr(),
                                       objf_ws.data_ptr(), stream()) == 0
    sync()
    t, s = R.xent_deriv64(p, labels)
    err = np.abs(Dm.get().astype(np.float64) - t)
    print(f"xent {case['name']}: worst |D - D64| / S_r = {(err / np.maximum(s, 1e-300)).max():.3e}")
    assert (err <= 1e-5 * s).all()
    objf64 = sum(float(F32(w)) * np.log(np.float64(p[i, c])) for i, c, w in labels)
    wsum = sum(float(F32(w)) for _, _, w in labels)
    got = tot.cpu().numpy()
    assert np.isnan(got[2:]).all() and np.isnan(objf_ws[objf_n:].cpu().numpy()).all()
    assert abs(got[0] - objf64) <= 1e-6 * abs(objf64)
    assert got[1] == wsum
    want = p.astype(np.float64).sum(axis=0) if case["stats"] else np.zeros(cols)
    check_stats_buffers(vs, ws, n, cols, want, case["name"])
    assert_bits(Pm.get(), p, "out_value")


@pytest.mark.parametrize("case", T.select("kn_comp_objf_and_deriv"), ids=T.name_of)
def test_comp_objf_and_deriv_layouts(kc, KN, case):
    import torch
    rows, cols, per_row = case["rows"], case["cols"], case["per_row"]
    r = rng(cols + per_row)
    p = R.softmax_prop64(r.standard_normal((rows, cols)) * 3).astype(F32)
    start = r.standard_normal((rows, cols)).astype(F32)
    labels = []
    for i in range(rows):
        edge = edge_columns(cols)[-min(per_row, 2):]
        others = [int(c) for c in r.choice(cols - 8, size=per_row - len(edge), replace=False)]
        labels += [(i, c, float(r.integers(1, 9)) / 8) for c in sorted(others + edge)]
    assert len(labels) == case["args"][0]
    el = [torch.from_numpy(np.array([l[k] for l in labels], t)).cuda()
          for k, t in ((0, np.int32), (1, np.int32), (2, F32))]
    Pm, Dm = place(kc, case["ops"][0], p), place(kc, case["ops"][1], start)
    nb = KN.kn_comp_objf_blocks(len(labels))
    objf_n = KN.kn_objf_ws(nb) // 8
    objf_ws = torch.full((objf_n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    tot = torch.full((2 + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    tot[:2] = 0
    assert KN.kn_comp_objf_and_deriv(el[0].data_ptr(), el[1].data_ptr(), el[2].data_ptr(),
                                     len(labels), Pm.ptr, Pm.dim, Dm.ptr, Dm.dim, tot.data_ptr(),
                                     objf_ws.data_ptr(), stream()) == 0
    sync()
    exp_d, exp_objf, exp_w = R.comp_objf_and_deriv32(p, labels, start)
    assert_same(Dm.get(), exp_d, "deriv += w / p")
    got = tot.cpu().numpy()
    assert np.isnan(got[2:]).all() and np.isnan(objf_ws[objf_n:].cpu().numpy()).all()
    assert abs(got[0] - exp_objf) <= 1e-6 * abs(exp_objf)
    assert got[1] == exp_w
    assert_bits(Pm.get(), p, "probs")
