"""NormalizeComponent on the GPU against the numpy fp64 restatement of
tests/normalize_ref.py (reference nnet2/nnet-component.cc:576-639).

Bars: the project's 1e-5 bound against fp64 (outputs: rtol 1e-5 and each
row's root-mean-square within 1e-5 of 1; derivatives: 1e-5 * the sum of
|terms|); bit-exact where the fp32 result is determined (the floor branch at
power-of-two sizes, rows next to a non-finite row, a row at another position
of another batch, in_deriv aliasing out_deriv, model files).

The widths cover the three kernel forms and their edges: a row in one wave's
registers (up to 4096 columns, 4 / 16 / 32 / 64 values a lane), a row in a
block's registers (4097 to 16384, 32 / 64 values a thread), the re-read form
beyond.  The *_layouts tests call the launchers directly on pitched operands
with sentinels, at the layouts of tests/nnet2_kernel_cases.py: every access
width (4, 2, 1 columns a lane) at every count of values a thread holds, either
side of each step (tests/test_nnet2_routes.py pins the kernel of each case)."""
import functools
import os

import numpy as np
import pytest

import nnet2_kernel_cases as T
import normalize_ref as R
from _pitched import assert_bits, place, stream, sync
from _util import assert_same, host, padded, rng
from _util import dev as _dev

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = os.path.join(GOLDEN, "models")
COLS = [1, 2, 63, 64, 65, 1000, 1152, 4000, 4096, 4097, 16000, 16384, 16385]
# either side of the steps in the values a thread holds (4 | 16 | 32 | 64 a lane, 32 | 64 a thread)
STEP_COLS = [256, 257, 1024, 1025, 2048, 2049, 8192, 8193]
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def dev(a):
    return _dev(np.array(a))  # a copy: the shared cases are read-only


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def new(kc, cols):
    return kc.Component.NewFromString(f"NormalizeComponent dim={cols}")


@functools.lru_cache(maxsize=None)
def case(rows, cols, seed=0):
    """N(0, 1) times a per-row scale drawn (log-uniformly) from 1e-6 ... 1e6,
    a N(0, 1) derivative, and their fp64 answers (computed once, read-only)."""
    r = rng(1000 * seed + cols + rows)
    x = (r.standard_normal((rows, cols)) * 10.0 ** r.uniform(-6, 6, size=(rows, 1))).astype(F32)
    dy = r.standard_normal((rows, cols)).astype(F32)
    t = R.prop64(x)
    d, terms = R.backprop64(x, dy)
    for a in (x, dy, t, d, terms):
        a.setflags(write=False)
    return x, dy, t, d, terms


def check_inputs_clear_of_floor_and_overflow(x):
    p = R.mean_square64(x)
    assert (p >= 2 * R.NORM_FLOOR).all(), p.min()
    assert ((x.astype(np.float64) ** 2).sum(axis=1) < FLT_MAX).all()


def check_prop(y, x, t, what):
    y64 = y.astype(np.float64)
    with np.errstate(invalid="ignore"):  # 0 / 0 at an exact zero of a ReLU output
        rel = np.abs(y64 - t) / np.abs(t)
    rms = np.sqrt(R.mean_square64(y64))
    print(f"normalize prop {what}: worst rel err {np.nanmax(rel):.3e}, "
          f"worst |rms - 1| {np.abs(rms - 1).max():.3e}")
    assert (np.abs(y64 - t) <= 1e-5 * np.abs(t)).all(), np.nanmax(rel)
    assert (np.abs(rms - 1) <= 1e-5).all()


def check_backprop(d, t, terms, what):
    err = np.abs(d.astype(np.float64) - t)
    print(f"normalize backprop {what}: worst err / sum|terms| = "
          f"{(err / np.maximum(terms, 1e-300)).max():.3e}")
    assert (err <= 1e-5 * terms).all()


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", [1, 70])
def test_normalize_propagate(kc, rows, cols):
    x, _, t, _, _ = case(rows, cols)
    check_inputs_clear_of_floor_and_overflow(x)
    c = new(kc, cols)
    assert c.Type() == "NormalizeComponent" and c.InputDim() == c.OutputDim() == cols
    check_prop(host(c.Propagate(dev(x))), x, t, (rows, cols))


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", [1, 70])
def test_normalize_backprop(kc, rows, cols):
    x, dy, _, t, terms = case(rows, cols)
    check_inputs_clear_of_floor_and_overflow(x)
    c = new(kc, cols)
    assert c.BackpropNeedsInput() and not c.BackpropNeedsOutput()
    xd, dyd = dev(x), dev(dy)
    # out_value=None: Backprop does not read it
    check_backprop(host(c.Backprop(xd, None, dyd, update=True)), t, terms, (rows, cols))
    vs, ds, cnt = c.NonlinearStats()
    assert vs.size == 0 and ds.size == 0 and cnt == 0
    assert_same(host(c.Backprop(xd, None, dyd, update=False)),
                host(c.Backprop(xd, None, dyd, update=True)), "update on / off")


@pytest.mark.parametrize("cols", STEP_COLS)
def test_normalize_at_register_steps(kc, cols):
    x, dy, t, d, terms = case(70, cols, seed=1)
    check_inputs_clear_of_floor_and_overflow(x)
    c = new(kc, cols)
    check_prop(host(c.Propagate(dev(x))), x, t, (70, cols))
    check_backprop(host(c.Backprop(dev(x), None, dev(dy))), d, terms, (70, cols))


@pytest.fixture(scope="module")
def KN(kc):
    return T.bind(kc)


@pytest.mark.parametrize("kcase", T.select("kn_normalize_prop"), ids=T.name_of)
def test_normalize_propagate_layouts(kc, KN, kcase):
    x, _, t, _, _ = case(kcase["rows"], kcase["cols"], seed=6)
    check_inputs_clear_of_floor_and_overflow(x)
    X, Y = place(kc, kcase["ops"][0], x), place(kc, kcase["ops"][1])
    assert KN.kn_normalize_prop(X.ptr, X.dim, Y.ptr, Y.dim, stream()) == 0
    sync()
    check_prop(Y.get(), x, t, kcase["name"])
    assert_bits(X.get(), x, "the input")


@pytest.mark.parametrize("kcase", T.select("kn_normalize_backprop"), ids=T.name_of)
def test_normalize_backprop_layouts(kc, KN, kcase):
    x, dy, _, t, terms = case(kcase["rows"], kcase["cols"], seed=6)
    X, E, D = place(kc, kcase["ops"][0], x), place(kc, kcase["ops"][1], dy), place(kc, kcase["ops"][2])
    assert KN.kn_normalize_backprop(X.ptr, X.dim, E.ptr, E.dim, D.ptr, D.dim, stream()) == 0
    sync()
    check_backprop(D.get(), t, terms, kcase["name"])
    assert_bits(X.get(), x, "in_value")
    assert_bits(E.get(), dy, "out_deriv")


@pytest.mark.parametrize("cols", [1, 64, 4096, 8192])
def test_normalize_floor_branch_exact(kc, cols):
    """1 / D and every sum here are exact in any order.  Row 0, +-2^-33, has
    p = 2^-66 = kNormFloor: on the floor branch (f = 2^33, g = 0); row 1, all
    zero, is floored; row 2, +-2^-32, is not and has both terms."""
    r = rng(cols)
    sign = np.where(r.random(cols) < 0.5, -1.0, 1.0).astype(F32)
    x = np.zeros((3, cols), F32)
    x[0] = sign * F32(2.0 ** -33)
    x[2] = sign * F32(2.0 ** -32)
    dy = r.standard_normal((3, cols)).astype(F32)
    assert R.mean_square64(x)[0] == R.NORM_FLOOR and R.mean_square64(x)[2] == 4 * R.NORM_FLOOR
    c = new(kc, cols)
    y = host(c.Propagate(dev(x)))
    assert (bits(y[0]) == bits(x[0] * F32(2.0 ** 33))).all() and (np.abs(y[0]) == 1).all()
    assert (bits(y[1]) == 0).all()
    assert (bits(y[2]) == bits(sign)).all()
    d = host(c.Backprop(dev(x), None, dev(dy)))
    assert (bits(d[:2]) == bits(dy[:2] * F32(2.0 ** 33))).all()
    t, terms = R.backprop64(x, dy)
    second = t[2] - 2.0 ** 32 * dy[2].astype(np.float64)
    assert (second != 0).all()  # the reference's row 2 has a second term at every element
    check_backprop(d[2:], t[2:], terms[2:], f"+-2^-32 at {cols}")


@pytest.mark.parametrize("cols,kind", [(64, "nan"), (64, "inf"), (64, "1e30"), (5000, "nan"),
                                       (5000, "inf"), (16385, "nan"), (16385, "inf")])
def test_normalize_propagate_nonfinite_row(kc, cols, kind):
    """The reference's product form: out = x * f with f = 0 for a row whose
    sum of squares is inf (1e30^2 overflows fp32), so inf * 0 = NaN at an inf
    entry and 0 elsewhere; a NaN makes f NaN.  No other row changes."""
    x = np.array(case(70, cols, seed=2)[0])
    c = new(kc, cols)
    clean = host(c.Propagate(dev(x)))
    at = min(17, cols - 1)
    x[3, at] = {"nan": np.nan, "inf": np.inf, "1e30": 1e30}[kind]
    y = host(c.Propagate(dev(x)))
    if kind == "nan":
        assert np.isnan(y[3]).all()
    elif kind == "inf":
        assert np.isnan(y[3, at])
        assert (np.delete(y[3], at) == 0).all()
    else:
        assert (y[3] == 0).all()
    keep = np.arange(70) != 3
    assert (bits(y[keep]) == bits(clean[keep])).all()


@pytest.mark.parametrize("cols", [1000, 4000, 16000, 16385])
def test_normalize_row_independence(kc, cols):
    """The same 3 rows as a 3-row batch and as rows 67-69 of a 70-row batch:
    identical bits both ways, and from one call to the next."""
    x3, dy3 = case(3, cols, seed=3)[:2]
    x70, dy70 = (np.array(a) for a in case(70, cols, seed=3)[:2])
    x70[67:], dy70[67:] = x3, dy3
    c = new(kc, cols)
    small = [(host(c.Propagate(dev(x3))), host(c.Backprop(dev(x3), None, dev(dy3))))
             for _ in range(2)]
    big = [(host(c.Propagate(dev(x70))), host(c.Backprop(dev(x70), None, dev(dy70))))
           for _ in range(2)]
    for k in (0, 1):
        assert (bits(small[0][k]) == bits(small[1][k])).all()
        assert (bits(big[0][k]) == bits(big[1][k])).all()
        assert (bits(small[0][k]) == bits(big[0][k][67:])).all()


@pytest.mark.parametrize("cols,extra", [(3454, 2), (3454, 0), (16001, 0)])
def test_normalize_strides(kc, cols, extra):
    """3454 columns at row stride 3456 (16-byte rows) and 3454 (odd rows only
    8-byte aligned), 16001 at stride 16001 (4-byte): every access width of
    the wave and block forms; the pad columns of the outputs stay untouched."""
    import torch
    x, dy, t, d64, terms = case(70, cols, seed=4)
    c = new(kc, cols)
    xd, dyd = padded(np.array(x), extra), padded(np.array(dy), extra)
    for run in ("prop", "backprop"):
        base = torch.full((70, cols + extra), float("nan"), dtype=torch.float32, device="cuda")
        out = base[:, :cols]
        assert xd.stride(0) == dyd.stride(0) == out.stride(0) == cols + extra
        if run == "prop":
            c.Propagate(xd, out=out)
            check_prop(host(out), x, t, (cols, extra))
        else:
            c.Backprop(xd, None, dyd, in_deriv=out)
            check_backprop(host(out), d64, terms, (cols, extra))
        assert torch.isnan(base[:, cols:]).all()


@pytest.mark.parametrize("cols", [1000, 16000, 16385])
def test_normalize_backprop_in_place(kc, cols):
    """in_deriv passed as the out_deriv tensor, on each of the three forms."""
    x, dy = case(70, cols, seed=5)[:2]
    c = new(kc, cols)
    xd = dev(x)
    apart = host(c.Backprop(xd, None, dev(dy)))
    both = dev(dy)
    ret = c.Backprop(xd, None, both, in_deriv=both)
    assert ret.data_ptr() == both.data_ptr()
    assert (bits(host(both)) == bits(apart)).all()


def test_normalize_model_io(kc, tmp_path):
    path = os.path.join(MODELS, "normalize.bin")
    z = np.load(os.path.join(MODELS, "normalize.npz"))
    c = kc.Component.ReadNew(path)
    assert c.Type() == "NormalizeComponent"
    assert c.InputDim() == c.OutputDim() == int(z["dim"]) == 12
    vs, ds, cnt = c.NonlinearStats()
    assert vs.size == 0 and ds.size == 0 and cnt == 0
    out = tmp_path / "normalize.bin"
    c.Write(out, True)
    assert open(out, "rb").read() == open(path, "rb").read()
    text = tmp_path / "normalize.txt"
    c.Write(text, False)
    again = kc.Component.ReadNew(text)
    assert again.Type() == "NormalizeComponent" and again.Info() == c.Info()
    assert again.NonlinearStats()[2] == 0
    again.Write(out, True)
    assert open(out, "rb").read() == open(path, "rb").read()
    x = dev(rng(6).standard_normal((5, 12)).astype(F32))
    y = host(c.Propagate(x))
    assert (bits(host(c.Copy().Propagate(x))) == bits(y)).all()
    assert (bits(host(again.Propagate(x))) == bits(y)).all()


FC = ("FullyConnectedComponent input-dim={i} output-dim={o} learning-rate=0.02 "
      "param-stddev={s} bias-stddev=0.5 weight-decay=0.0005 momentum=0.9")
SMALL = "\n".join([
    "SpliceComponent input-dim=8 left-context=2 right-context=2 const-component-dim=0",
    "ConvolutionComponent in-height=8 in-width=5 in-channel=1 kernel-height=8 kernel-width=2 "
    "stride=1 group=32 out-height=1 out-width=4 learning-rate=0.02 param-stddev=0.3 "
    "bias-stddev=0.5 weight-decay=0.0005 momentum=0.9",
    "MaxpoolComponent in-height=1 in-width=4 in-channel=32 pool-height-dim=1 pool-width-dim=2 "
    "pool-channel-dim=1",
    "RectifiedLinearComponent dim=64",
    "NormalizeComponent dim=64",
    FC.format(i=64, o=16, s=0.3),
    "RectifiedLinearComponent dim=16",
    "NormalizeComponent dim=16",
    FC.format(i=16, o=10, s=0.3),
    "SoftmaxComponent dim=10"])


def test_normalize_in_a_stack(kc):
    """The train_conv topology, small: each Normalize layer's output and input
    derivative against the fp64 restatement of what the stack itself fed it
    (the output of the layer below, the derivative from the layer above), so
    the runtime kept the Normalize input alive until its Backprop."""
    kc.set_randn_seed(81)
    net = kc.Nnet(SMALL)
    types = [c.Type() for c in net.components]
    norms = [i for i, t in enumerate(types) if t == "NormalizeComponent"]
    assert norms == [4, 7]
    r = rng(13)
    x = dev(r.standard_normal((6 * 5, 8)).astype(F32))
    labels = [(i, int(r.integers(10)), 1.0) for i in range(6)]
    net.Propagate(x)
    below = {}
    for i in norms:
        below[i] = host(net.Output(i - 1))
        assert below[i].shape == (6, net.components[i].InputDim())
        check_prop(host(net.Output(i)), below[i], R.prop64(below[i]), f"stack layer {i}")
    net.BackpropXent(labels)
    objf, w = net.ObjfTotal()
    assert w == 6 and np.isfinite(objf) and objf < 0
    for i in norms:
        above = host(net.InputDeriv(i + 1))
        assert np.abs(above).max() > 0
        # the input is still what Propagate left there
        assert (bits(host(net.Output(i - 1))) == bits(below[i])).all()
        t, terms = R.backprop64(below[i], above)
        check_backprop(host(net.InputDeriv(i)), t, terms, f"stack layer {i}")
    assert all(net.components[i].NonlinearStats()[2] == 0 for i in norms)


def train_conv_step(kc):
    kc.set_randn_seed(2027)
    net = kc.Nnet(open(os.path.join(GOLDEN, "train_conv.config")).read())
    r = rng(14)
    x = dev(r.standard_normal((8 * 21, 40)).astype(F32))
    labels = [(i, int(r.integers(3454)), 1.0) for i in range(8)]
    net.Propagate(x)
    net.BackpropXent(labels)
    objf, w = net.ObjfTotal()
    params = [host(c.GetParam(which)) for c in net.components
              if c.Type() in ("ConvolutionComponent", "FullyConnectedComponent")
              for which in (kc.PARAM_LINEAR, kc.PARAM_BIAS)]
    return net, objf, w, params


def test_train_conv_config_trains_a_step(kc):
    net, objf, w, params = train_conv_step(kc)
    assert net.NumComponents() == 10
    assert [c.Type() for c in net.components][4::3] == ["NormalizeComponent"] * 2
    # the last FC starts at zero: every output 1 / 3454 (as for nnet.config)
    assert w == 8 and np.isfinite(objf)
    assert abs(objf - (-8 * np.log(3454.0))) <= 1e-6 * 8 * np.log(3454.0)
    assert len(params) == 6 and all(np.isfinite(p).all() for p in params)
    _, objf2, w2, params2 = train_conv_step(kc)
    assert (objf2, w2) == (objf, w)
    for a, b in zip(params, params2):
        assert (bits(a) == bits(b)).all()
