"""CPU checks behind tests/test_gpu_normalize.py: the numpy restatement of
normalize_ref.py against torch fp64 autograd, its floor branch, and the
NormalizeComponent model fixture against its encoder."""
import os

import numpy as np
import pytest

import kaldi_binary_normalize as KBN
import normalize_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = os.path.join(GOLDEN, "models")


@pytest.mark.parametrize("cols", [1, 7, 64, 1000])
def test_backprop64_is_the_autograd_derivative(cols):
    import torch
    r = np.random.default_rng(cols)
    x = r.standard_normal((5, cols)) * 10.0 ** r.uniform(-3, 3, size=(5, 1))
    dy = r.standard_normal((5, cols))
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    p = (xt * xt).mean(dim=1, keepdim=True)
    y = xt / torch.sqrt(torch.clamp(p, min=R.NORM_FLOOR))
    np.testing.assert_allclose(R.prop64(x), y.detach().numpy(), rtol=1e-13)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    d, terms = R.backprop64(x, dy)
    assert (np.abs(d - xt.grad.numpy()) <= 1e-12 * terms).all()
    # every output row has root-mean-square 1
    np.testing.assert_allclose(R.mean_square64(R.prop64(x)), 1.0, rtol=1e-13)


def test_zero_row_derivative_is_the_floor_scale():
    dy = np.random.default_rng(0).standard_normal((3, 16))
    x = np.zeros((3, 16))
    assert (R.prop64(x) == 0).all()
    d, terms = R.backprop64(x, dy)
    assert (d == 2.0 ** 33 * dy).all()
    assert (terms == 2.0 ** 33 * np.abs(dy)).all()


def test_floor_rule():
    """p == kNormFloor is on the floor branch (g = 0); twice the amplitude is
    not, and has the full two-term derivative."""
    s = np.where(np.arange(64) % 2 == 0, 1.0, -1.0)[None, :]
    dy = np.random.default_rng(1).standard_normal((1, 64))
    on = s * 2.0 ** -33
    assert R.mean_square64(on)[0] == R.NORM_FLOOR
    f, g = R.scale64(on)
    assert f[0, 0] == 2.0 ** 33 and g[0, 0] == 0.0
    assert (R.backprop64(on, dy)[0] == 2.0 ** 33 * dy).all()
    off = s * 2.0 ** -32
    f, g = R.scale64(off)
    assert f[0, 0] == 2.0 ** 32 and g[0, 0] == 2.0 ** 96
    d, _ = R.backprop64(off, dy)
    expect = 2.0 ** 32 * (dy - (dy * s).sum() / 64 * s)
    np.testing.assert_allclose(d, expect, rtol=1e-12, atol=1e-3)


def test_fixture_matches_spec_encoder():
    z = np.load(os.path.join(MODELS, "normalize.npz"))
    params = {k: z[k] for k in z.files}
    assert int(params["dim"]) == 12 and float(params["count"]) == 0.0
    assert params["value_sum"].size == 0 and params["deriv_sum"].size == 0
    data = open(os.path.join(MODELS, "normalize.bin"), "rb").read()
    assert data == KBN.encode("normalize", params)
    assert data.startswith(b"\x00B<")


def test_train_conv_settings_file():
    lines = [l for l in open(os.path.join(GOLDEN, "train_conv.config")).read().splitlines()
             if l.strip()]
    assert [l.split()[0] for l in lines] == [
        "SpliceComponent", "ConvolutionComponent", "MaxpoolComponent",
        "RectifiedLinearComponent", "NormalizeComponent", "FullyConnectedComponent",
        "RectifiedLinearComponent", "NormalizeComponent", "FullyConnectedComponent",
        "SoftmaxComponent"]
    assert lines[4] == "NormalizeComponent dim=1152" and lines[7] == "NormalizeComponent dim=1024"
