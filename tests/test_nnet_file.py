"""Whole-network model files and the test model.

tests/golden/models/nnet_small.bin is one small network in the <Nnet> layout
of upstream Nnet::Write, encoded by tests/kaldi_binary_nnet.py (independent of
the C++ I/O) by scripts/make_model_fixtures_nnet.py; it holds every component
kind that has an encoder.  CPU: the fixture is what the encoder produces, and
the new entry points are declared.  GPU: Nnet.Read / Write round trips (binary
byte for byte, text, and a network built from a config), malformed files as
errors, and Nnet.Copy with --scales and --remove-dropout (nnet-am-copy), which
makes the test model of the dropout recipes.
"""
import os

import numpy as np
import pytest

import kaldi_binary_nnet as KBN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "models", "nnet_small.bin")
NEW_FUNCTIONS = ["kcnn_nnet_read", "kcnn_nnet_write", "kcnn_nnet_copy",
                 "kcnn_nnet_compute_prob", "kcnn_nnet_prob_total", "kcnn_comp_objf_accuracy"]
PARAMS = (0, 1, 2)  # kcnn.PARAM_LINEAR, PARAM_BIAS, PARAM_PREV_GRAD


def fixture_components():
    return KBN.from_npz(np.load(os.path.join(GOLDEN, "models", "nnet_small.npz")))


def test_fixture_matches_spec_encoder():
    comps = fixture_components()
    data = open(FIXTURE, "rb").read()
    assert data == KBN.encode(comps)
    assert data.startswith(b"\x00B<Nnet> <NumComponents> \x04\x09\x00\x00\x00<Components> <Splice")
    assert data.endswith(b"</SoftmaxComponent> </Components> </Nnet> ")
    assert [k for k, _ in comps] == ["splice", "conv", "maxpool", "relu", "normalize", "fc",
                                     "dropout", "fc", "softmax"]
    assert len(data) < 8192


def test_new_functions_declared():
    import kcnn
    names = kcnn.declared_symbols()
    for f in NEW_FUNCTIONS:
        assert f in names, f


# ---- GPU ------------------------------------------------------------------------
def updatable(net):
    return [c for c in net.components if c.NumGradientParams() > 0]


def params(c):
    from _util import host
    return [host(c.GetParam(w)) for w in PARAMS]


def shape_of(net):
    return [(c.Type(), c.InputDim(), c.OutputDim()) for c in net.components]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def fixture_input(rows=5, seed=3):
    """`rows` chunks of the fixture network's 3-frame context."""
    from _util import dev
    return dev(np.random.default_rng(seed).standard_normal((3 * rows, 8)).astype(np.float32))


@pytest.mark.gpu
def test_binary_round_trip(kc, tmp_path):
    from _util import host
    comps = fixture_components()
    net = kc.Nnet.Read(FIXTURE)
    assert net.NumComponents() == len(comps)
    assert [c.Type() for c in net.components] == [KBN.TYPES[k] for k, _ in comps]
    for c, (kind, p) in zip(net.components, comps):
        if kind in ("conv", "fc"):
            for got, key in zip(params(c), ("linear", "b", "prev")):
                assert (bits(got.reshape(p[key].shape)) == bits(p[key])).all(), (kind, key)
            assert c.LearningRate() == np.float32(p["lr"])
            rows, cols = p["linear"].shape
            if kind == "fc":
                assert (c.InputDim(), c.OutputDim()) == (cols, rows)
            else:
                assert c.InputDim() == int(p["H"]) * int(p["W"]) * int(p["C"])
                assert c.OutputDim() == int(p["oh"]) * int(p["ow"]) * int(p["G"])
        elif kind == "maxpool":
            assert (c.InputDim(), c.OutputDim()) == (int(p["input_dim"]), int(p["output_dim"]))
        elif kind in ("relu", "softmax", "normalize"):
            vs, ds, cnt = c.NonlinearStats()
            np.testing.assert_array_equal(vs, p["value_sum"])
            np.testing.assert_array_equal(ds, p["deriv_sum"])
            assert cnt == float(p["count"]) and c.InputDim() == c.OutputDim() == int(p["dim"])
        elif kind == "splice":
            assert c.Context() == list(p["context"]) and c.InputDim() == int(p["input_dim"])
            assert c.OutputDim() == int(p["input_dim"]) * len(p["context"])
        else:
            assert kind == "dropout" and c.InputDim() == int(p["dim"])
            assert c.Info().endswith("dropout_proportion = 0.5, dropout_scale = 0")
    out = tmp_path / "copy.bin"
    net.Write(out, binary=True)
    assert open(out, "rb").read() == open(FIXTURE, "rb").read()
    # and it runs
    net.Propagate(fixture_input())
    y = host(net.Output())
    assert y.shape == (5, 7) and np.isfinite(y).all()


@pytest.mark.gpu
def test_text_round_trip(kc, tmp_path):
    net = kc.Nnet.Read(FIXTURE)
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    net.Write(a, binary=False)
    text = open(a, "rb").read()
    assert text.startswith(b"<Nnet> <NumComponents> 9 <Components> <SpliceComponent> ")
    assert text.endswith(b"\n</Components> </Nnet> ")  # a newline after each component
    back = kc.Nnet.Read(a)
    assert shape_of(back) == shape_of(net)
    back.Write(b, binary=False)
    assert open(b, "rb").read() == text
    # text holds every fp32 exactly: the binary file comes back too
    c = tmp_path / "c.bin"
    back.Write(c, binary=True)
    assert open(c, "rb").read() == open(FIXTURE, "rb").read()


@pytest.mark.gpu
def test_config_round_trip(kc, tmp_path):
    """tests/golden/train_conv.config, written and read back, propagates a
    3-chunk input to the same bits (its last FC starts at zero: perturbed so
    that the output depends on everything below)."""
    from _util import dev, host
    kc.set_randn_seed(31)
    net = kc.Nnet(open(os.path.join(GOLDEN, "train_conv.config")).read())
    net.components[-2].PerturbParams(0.1)
    path = tmp_path / "train_conv.nnet"
    net.Write(path)
    back = kc.Nnet.Read(path)
    assert shape_of(back) == shape_of(net)
    x = dev(np.random.default_rng(4).standard_normal((3 * 21, 40)).astype(np.float32))
    net.Propagate(x)
    want = [host(net.Output(i)).copy() for i in (4, net.NumComponents() - 1)]
    back.Propagate(x)
    got = [host(back.Output(i)) for i in (4, back.NumComponents() - 1)]
    assert want[1].shape == (3, 3454) and len(np.unique(want[1])) > 100
    for w, g in zip(want, got):
        assert (bits(w) == bits(g)).all()


def _truncated(tmp_path):
    data = open(FIXTURE, "rb").read()
    p = tmp_path / "half.bin"
    p.write_bytes(data[:len(data) // 2])
    return p


def _count_raised(tmp_path):
    comps = fixture_components()
    p = tmp_path / "count.bin"
    p.write_bytes(KBN.encode(comps, num_components=len(comps) + 1))
    return p


def _fc_mismatch(tmp_path):
    comps = fixture_components()
    kind, fc2 = comps[7]
    assert kind == "fc" and comps[5][0] == "fc"
    wide = dict(fc2)
    wide["linear"] = np.zeros((7, 11), np.float32)  # the FC below gives 10
    wide["prev"] = np.zeros((7, 11), np.float32)
    comps[7] = (kind, wide)
    p = tmp_path / "mismatch.bin"
    p.write_bytes(KBN.encode(comps))
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("make", [_truncated, _count_raised, _fc_mismatch])
def test_malformed_file_is_an_error(kc, tmp_path, make):
    with pytest.raises(kc.KcnnError):
        kc.Nnet.Read(make(tmp_path))
    with pytest.raises(kc.KcnnError):
        kc.Nnet.Read(tmp_path / "no_such_file.bin")
    # the library goes on working
    assert kc.Nnet.Read(FIXTURE).NumComponents() == 9


@pytest.mark.gpu
def test_malformed_tokens_are_errors(kc, tmp_path):
    data = open(FIXTURE, "rb").read()
    cases = {"unknown component": data.replace(b"<SoftmaxComponent>", b"<SoftminComponent>"),
             "missing <Components>": data.replace(b"<Components> ", b"", 1),
             "missing </Nnet>": data[:-len(b"</Nnet> ")],
             "no components": KBN.encode([]),
             "count lowered": KBN.encode(fixture_components(), num_components=8)}
    for what, blob in cases.items():
        p = tmp_path / "bad.bin"
        p.write_bytes(blob)
        print(what)
        with pytest.raises(kc.KcnnError):
            kc.Nnet.Read(p)


@pytest.mark.gpu
def test_copy_scales(kc):
    net = kc.Nnet.Read(FIXTURE)
    ups = updatable(net)
    assert [c.Type() for c in ups] == ["ConvolutionComponent", "FullyConnectedComponent",
                                       "FullyConnectedComponent"]
    before = [params(c) for c in ups]
    scales = [0.5, 4.0, 0.125]
    copy = kc.Nnet.Copy(net, scales=scales)
    assert shape_of(copy) == shape_of(net)
    for c, orig, s in zip(updatable(copy), ups, scales):
        ref = orig.Copy()
        ref.Scale(s)
        for got, want in zip(params(c), params(ref)):
            assert (bits(got) == bits(want)).all()
        assert (bits(params(c)[0]) == bits(params(orig)[0] * np.float32(s))).all()
        assert (bits(params(c)[1]) == bits(params(orig)[1] * np.float32(s))).all()
    for c, orig in zip(copy.components, net.components):
        if c.NumGradientParams() == 0:
            assert c.Info() == orig.Info()
            if c.Type() in ("RectifiedLinearComponent", "SoftmaxComponent"):
                for a, b in zip(c.NonlinearStats(), orig.NonlinearStats()):
                    np.testing.assert_array_equal(a, b)
    for bad in ([0.5, 4.0], [0.5, 4.0, 0.125, 1.0], []):
        with pytest.raises(kc.KcnnError, match="scales"):
            net.Copy(scales=bad)
    for c, want in zip(ups, before):
        for got, w in zip(params(c), want):
            assert (bits(got) == bits(w)).all(), "the original changed"
    # no arguments: a plain deep copy, which does not alias the original
    plain = net.Copy()
    assert shape_of(plain) == shape_of(net)
    for c, want in zip(updatable(plain), before):
        for got, w in zip(params(c), want):
            assert (bits(got) == bits(w)).all()
    updatable(plain)[0].Scale(2.0)
    assert (bits(params(ups[0])[0]) == bits(before[0][0])).all()


@pytest.mark.gpu
def test_copy_remove_dropout(kc):
    from _util import host
    net = kc.Nnet.Read(FIXTURE)
    test_model = net.Copy(remove_dropout=True)
    assert test_model.NumComponents() == net.NumComponents() - 1
    assert "DropoutComponent" not in [c.Type() for c in test_model.components]
    assert shape_of(test_model) == [s for s in shape_of(net) if s[0] != "DropoutComponent"]
    # no mask is drawn: the test model repeats, the original does not
    x = fixture_input(rows=40)
    outs = []
    for n in (test_model, test_model, net, net):
        n.Propagate(x)
        outs.append(host(n.Output()).copy())
    assert (bits(outs[0]) == bits(outs[1])).all()
    assert not (bits(outs[2]) == bits(outs[3])).all()


@pytest.mark.gpu
def test_nnet_config_test_model(kc):
    """The recipes' step after training: nnet-am-copy --scales=$dropout_scale
    --remove-dropout=true on the reference's own network."""
    from _util import dev, host
    scales = [float(s) for s in
              open(os.path.join(GOLDEN, "dropout_scale.config")).read().strip().split(":")]
    assert scales == [1, 1, 1, 1, 1, 1, 0.5, 0.5, 1]
    kc.set_randn_seed(2027)
    net = kc.Nnet(open(os.path.join(GOLDEN, "nnet.config")).read())
    net.components[-2].PerturbParams(0.05)  # the last FC starts at zero
    test_model = net.Copy(scales=scales, remove_dropout=True)
    assert (net.NumComponents(), test_model.NumComponents()) == (22, 20)
    assert "DropoutComponent" not in [c.Type() for c in test_model.components]
    ups, tups = updatable(net), updatable(test_model)
    assert len(ups) == len(tups) == 9
    for k in (6, 7):
        assert tups[k].Type() == "FullyConnectedComponent"
        for w in (0, 1):
            got, orig = host(tups[k].GetParam(w)), host(ups[k].GetParam(w))
            assert np.abs(orig).max() > 0
            assert (bits(got) == bits(orig * np.float32(0.5))).all(), (k, w)
    for k in (0, 5, 8):
        assert (bits(host(tups[k].GetParam(0))) == bits(host(ups[k].GetParam(0)))).all()
    x = dev(np.random.default_rng(11).standard_normal((8 * 21, 40)).astype(np.float32))
    outs = []
    for n in (test_model, test_model, net, net):
        n.Propagate(x)
        outs.append(host(n.Output()).copy())
    assert outs[0].shape == (8, 3454)
    assert (bits(outs[0]) == bits(outs[1])).all()
    assert not (bits(outs[2]) == bits(outs[3])).all()
