"""Model arithmetic of the updatable components over the C ABI (Scale, Add,
DotProduct, SetZero, PerturbParams: what model combination and
Nnet.Copy(scales=...) rest on), and the plain nnet2 AffineComponent, which
no network of the other tests contains: Propagate, Backprop, its update
rule, Write / Read and the parameter-gradient identity through DotProduct.

References are numpy, float32 for single operations (bit equality) and fp64
otherwise.  The components: a ConvolutionComponent (CONVS["small_pad"]: 18 x
5 kernel matrix), a FullyConnectedComponent and an AffineComponent, both
300 -> 70.

Add / DotProduct across types follow each class's dynamic_cast: a
FullyConnectedComponent is an AffineComponent, so FC.Add(Affine) and
Affine.Add(FC) both work (linear and bias parameters; the FC's prev_grad
takes no part); a ConvolutionComponent accepts only its own type.
"""
import re

import numpy as np
import pytest

from _util import assert_bound, dev, host, randn, rng
from test_gpu_components import CONVS, conv_line

pytestmark = pytest.mark.gpu

IN, OUT = 300, 70
LINES = {
    "conv": conv_line(*CONVS["small_pad"]),
    "fc": (f"FullyConnectedComponent input-dim={IN} output-dim={OUT} learning-rate=0.01 "
           "weight-decay=0.0005 momentum=0.5"),
    "affine": f"AffineComponent input-dim={IN} output-dim={OUT} learning-rate=0.01",
}
KINDS = list(LINES)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:3]}"


def n_params(kc, comp):
    return 3 if comp.Type() != "AffineComponent" else 2   # (no prev_grad)


def get(kc, comp):
    return [host(comp.GetParam(w)) for w in range(n_params(kc, comp))]


def build(kc, kind, seed, integer=False):
    """The component with parameters (and prev_grad) set from numpy."""
    comp = kc.Component.NewFromString(LINES[kind])
    r = rng(seed)
    vals = []
    for which in range(n_params(kc, comp)):
        shape = comp.ParamDim(which)
        v = (r.integers(-8, 9, size=shape).astype(np.float32) if integer
             else randn(r, shape, (0.1, 0.5, 0.01)[which]))
        comp.SetParam(which, dev(v))
        vals.append(v.reshape(-1) if which == kc.PARAM_BIAS else v)
    return comp, vals


@pytest.mark.parametrize("s", [0.5, -3.0, 0.0])
@pytest.mark.parametrize("kind", KINDS)
def test_scale(kc, kind, s):
    comp, p = build(kc, kind, 1)
    lr = comp.LearningRate()
    comp.Scale(s)
    got = get(kc, comp)
    same_bits(got[0], p[0] * np.float32(s), "linear")
    same_bits(got[1], p[1] * np.float32(s), "bias")
    if len(p) == 3:
        same_bits(got[2], p[2], "prev_grad")
    assert comp.LearningRate() == lr


@pytest.mark.parametrize("kind", KINDS)
def test_add(kc, kind):
    a, p = build(kc, kind, 2)
    b, q = build(kc, kind, 3)
    alpha = np.float32(-0.7)
    a.Add(float(alpha), b)
    got = get(kc, a)
    for k, what in enumerate(("linear", "bias")):
        aq = np.float64(alpha) * q[k].astype(np.float64)
        err = np.abs(got[k] - (aq + p[k]))
        lim = 2.0 ** -23 * (np.abs(aq) + np.abs(p[k]))
        assert (err <= lim).all(), f"{what}: worst err/bound {(err / lim).max():.3f}"
    if len(p) == 3:
        same_bits(got[2], p[2], "prev_grad")
    for g_, q_ in zip(get(kc, b), q):
        same_bits(g_, q_, "other")
    # representable: integers and a power of two
    a, p = build(kc, kind, 4, integer=True)
    b, q = build(kc, kind, 5, integer=True)
    a.Add(0.25, b)
    got = get(kc, a)
    same_bits(got[0], p[0] + np.float32(0.25) * q[0], "exact linear")
    same_bits(got[1], p[1] + np.float32(0.25) * q[1], "exact bias")
    # a + a
    a, p = build(kc, kind, 6)
    a.Add(1.0, a.Copy())
    got = get(kc, a)
    same_bits(got[0], 2 * p[0], "doubled linear")
    same_bits(got[1], 2 * p[1], "doubled bias")


def test_add_mismatch(kc):
    conv, pc = build(kc, "conv", 7)
    fc, pf = build(kc, "fc", 8)
    small = kc.Component.NewFromString(
        "FullyConnectedComponent input-dim=20 output-dim=7 learning-rate=0.01 "
        "weight-decay=0.0005 momentum=0.5")
    conv2 = kc.Component.NewFromString(conv_line(3, 4, 1, 2, 2, 3, 0, 0))
    for a, other, before in ((conv, fc, pc), (fc, conv, pf), (fc, small, pf), (conv, conv2, pc)):
        with pytest.raises(kc.KcnnError):
            a.Add(0.5, other)
        with pytest.raises(kc.KcnnError):
            a.DotProduct(other)
        for g_, p_ in zip(get(kc, a), before):
            same_bits(g_, p_, f"{a.Type()} after a rejected Add")


def test_add_fc_affine(kc):
    """AffineComponent::Add casts the other to AffineComponent, which a
    FullyConnectedComponent is: both directions add linear and bias."""
    for first, second in (("fc", "affine"), ("affine", "fc")):
        a, p = build(kc, first, 9, integer=True)
        b, q = build(kc, second, 10, integer=True)
        a.Add(2.0, b)
        got = get(kc, a)
        same_bits(got[0], p[0] + 2 * q[0], f"{first} += 2 {second}: linear")
        same_bits(got[1], p[1] + 2 * q[1], f"{first} += 2 {second}: bias")
        if len(p) == 3:
            same_bits(got[2], p[2], "prev_grad")
        t = float((p[0].astype(np.float64) + 2 * q[0]).ravel() @ q[0].astype(np.float64).ravel()
                  + (p[1].astype(np.float64) + 2 * q[1]) @ q[1].astype(np.float64))
        assert a.DotProduct(b) == t and b.DotProduct(a) == t


def dot64(p, q):
    tw = float(np.sum(p[0].astype(np.float64) * q[0]))
    tb = float(np.sum(p[1].astype(np.float64) * q[1]))
    return tw, tb


@pytest.mark.parametrize("kind", KINDS)
def test_dot_product(kc, kind):
    a, p = build(kc, kind, 11)
    b, q = build(kc, kind, 12)
    tw, tb = dot64(p, q)
    got = a.DotProduct(b)
    # the two sums come back as floats and are added in float
    assert abs(got - (tw + tb)) <= 2.0 ** -22 * (abs(tw) + abs(tb)), (got, tw, tb)
    assert b.DotProduct(a) == got
    ai, pi = build(kc, kind, 13, integer=True)
    bi, qi = build(kc, kind, 14, integer=True)
    tw, tb = dot64(pi, qi)
    assert ai.DotProduct(bi) == tw + tb and tw != 0
    # with itself: Info()'s standard deviations, printed to 6 digits
    info = a.Info()
    ls = float(re.search(r"linear-params-stddev=([^,]+)", info).group(1))
    bs = float(re.search(r"bias-params-stddev=([^,]+)", info).group(1))
    tw, tb = dot64(p, p)
    nw, nb = p[0].size, p[1].size
    digits = 5e-6 + 2.0 ** -24          # half a unit of the 6th digit; the float sum
    assert abs(ls - np.sqrt(tw / nw)) <= digits * np.sqrt(tw / nw), info
    assert abs(bs - np.sqrt(tb / nb)) <= digits * np.sqrt(tb / nb), info
    self_dot = a.DotProduct(a)
    assert abs(self_dot - (tw + tb)) <= 2.0 ** -22 * (tw + tb)
    printed = nw * ls * ls + nb * bs * bs
    assert abs(self_dot - printed) <= (2 * digits * (1 + digits) + 2.0 ** -22) * printed


@pytest.mark.parametrize("as_gradient", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_set_zero(kc, kind, as_gradient):
    comp, p = build(kc, kind, 15)
    lr = comp.LearningRate()
    assert lr != 1.0
    comp.SetZero(as_gradient)
    got = get(kc, comp)
    assert not bits(got[0]).any() and not bits(got[1]).any()   # +0 everywhere
    if len(p) == 3:
        same_bits(got[2], p[2], "prev_grad")
    assert comp.LearningRate() == (1.0 if as_gradient else lr)


@pytest.mark.parametrize("kind", KINDS)
def test_perturb_params(kc, kind):
    comp, p = build(kc, kind, 16)
    twin = comp.Copy()
    stddev = np.float32(0.5)
    kc.set_randn_seed(1234)
    comp.PerturbParams(float(stddev))
    kc.set_randn_seed(1234)
    twin.PerturbParams(float(stddev))
    got = get(kc, comp)
    for g_, t_ in zip(got, get(kc, twin)):
        same_bits(g_, t_, "the same seed")
    if len(p) == 3:
        same_bits(got[2], p[2], "prev_grad")
    zw = (got[0].astype(np.float64) - p[0]) / float(stddev)
    zb = (got[1].astype(np.float64) - p[1]) / float(stddev)
    assert np.abs(zw).max() > 0 and np.abs(zb).max() > 0
    # the bias has draws of its own
    k = min(zb.size, zw.size)
    assert np.abs(zb[:k] - zw.ravel()[:k]).max() > 0.1
    if kind == "fc":
        n = zw.size
        assert n == 21000
        # five sigma of a fixed seed's sample mean and variance
        assert abs(zw.mean()) <= 5 / np.sqrt(n), zw.mean()
        assert abs(zw.var() - 1) <= 5 * np.sqrt(2 / n), zw.var()
    still, p = build(kc, kind, 17)
    still.PerturbParams(0.0)
    for g_, p_ in zip(get(kc, still), p):
        same_bits(g_, p_, "stddev 0")


# ---- AffineComponent ------------------------------------------------------------
def affine_data(N, seed):
    r = rng(seed)
    return randn(r, (N, IN)), randn(r, (N, OUT), 0.1)


@pytest.mark.parametrize("N", [33, 470])
def test_affine_propagate_backprop(kc, N):
    comp, (W, b) = build(kc, "affine", 20 + N)
    assert comp.Type() == "AffineComponent" and (comp.InputDim(), comp.OutputDim()) == (IN, OUT)
    lr = comp.LearningRate()
    x, dy = affine_data(N, 21 + N)
    x64, dy64, W64, b64 = (v.astype(np.float64) for v in (x, dy, W, b))
    y = comp.Propagate(dev(x))
    assert_bound(host(y), x64 @ W64.T + b64, np.abs(x64) @ np.abs(W64).T + np.abs(b64),
                 what="Affine Propagate")
    dx = comp.Backprop(dev(x), None, dev(dy), update=False)
    assert_bound(host(dx), dy64 @ W64, np.abs(dy64) @ np.abs(W64), what="Affine Backprop dX")
    for g_, p_ in zip(get(kc, comp), (W, b)):
        same_bits(g_, p_, "Backprop without update")
    # nnet2's rule (UpdateSimple): W += lr dY^T X, b += lr colsum(dY), no 1 / N
    dx2 = comp.Backprop(dev(x), None, dev(dy), update=True)
    assert_bound(host(dx2), dy64 @ W64, np.abs(dy64) @ np.abs(W64), what="Affine Backprop dX (update)")
    W1, b1 = get(kc, comp)
    assert_bound(W1, W64 + lr * (dy64.T @ x64), np.abs(W64) + lr * (np.abs(dy64).T @ np.abs(x64)),
                 what="Affine W update")
    assert_bound(b1, b64 + lr * dy64.sum(0), np.abs(b64) + lr * np.abs(dy64).sum(0),
                 what="Affine b update")
    assert comp.LearningRate() == lr


@pytest.mark.parametrize("binary", [True, False])
def test_affine_write_read(kc, tmp_path, binary):
    comp, (W, b) = build(kc, "affine", 30)
    p = tmp_path / ("affine.bin" if binary else "affine.txt")
    comp.Write(p, binary)
    back = kc.Component.ReadNew(p)
    assert back.Type() == "AffineComponent" and back.Info() == comp.Info()
    assert back.LearningRate() == comp.LearningRate()
    got = get(kc, back)
    same_bits(got[0], W, "linear")
    same_bits(got[1], b, "bias")


@pytest.mark.parametrize("N", [33, 470])
def test_affine_gradient_dot_product(kc, N):
    """The layer is linear in its parameters: for a perturbation d of them,
    sum((Propagate_{W+d}(x) - Propagate_W(x)) w) = <gradient, d> with no
    step-size slack.  The gradient is a copy's own accumulation: SetZero(True)
    (zero parameters, learning rate 1, the gradient flag) and a Backprop with
    update hold dY^T X and colsum(dY)."""
    comp, (W, b) = build(kc, "affine", 40 + N)
    x, w = affine_data(N, 41 + N)
    g = comp.Copy()
    g.SetZero(True)
    g.Backprop(dev(x), None, dev(w), update=True)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    gW, gb = get(kc, g)
    assert_bound(gW, w64.T @ x64, np.abs(w64).T @ np.abs(x64), what="accumulated dY^T X")
    assert_bound(gb, w64.sum(0), np.abs(w64).sum(0), what="accumulated colsum(dY)")
    # a perturbation of the parameters' own size
    d, (dW, db) = build(kc, "affine", 42 + N)
    dW64, db64 = dW.astype(np.float64), db.astype(np.float64)
    pred = g.DotProduct(d)
    # in fp64 from the inputs; S: the sum's |terms| (each gradient element is
    # held to 1e-5 of its own S, and meets |d|)
    t = float(((x64 @ dW64.T + db64) * w64).sum())
    S = float(((np.abs(x64) @ np.abs(dW64).T + np.abs(db64)) * np.abs(w64)).sum())
    assert abs(pred - t) <= 1e-5 * S, (pred, t, abs(pred - t) / S)
    # and as the library's own Propagate sees it; that difference of two
    # outputs carries both outputs' error scales
    moved = comp.Copy()
    moved.SetParam(kc.PARAM_LINEAR, dev(W + dW))
    moved.SetParam(kc.PARAM_BIAS, dev(b + db))
    y0, y1 = host(comp.Propagate(dev(x))).astype(np.float64), host(moved.Propagate(dev(x))).astype(np.float64)
    obs = float(((y1 - y0) * w64).sum())
    S2 = sum(float(((np.abs(x64) @ np.abs(A.astype(np.float64)).T + np.abs(c.astype(np.float64)))
                    * np.abs(w64)).sum()) for A, c in ((W, b), (W + dW, b + db)))
    assert abs(pred - obs) <= 1e-5 * (S + S2), (pred, obs, abs(pred - obs) / (S + S2))
