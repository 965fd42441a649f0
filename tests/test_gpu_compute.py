"""Nnet.Compute: the whole-utterance forward pass of upstream NnetComputer
(nnet-am-compute, the decodable) over a batch of utterances, on the GPU.

Yardstick.  For a network whose only SpliceComponent is component 0, the
window matrix Propagate takes today is built in numpy -- frame t of utterance
u is the rows X_u[clamp(t + o, 0, T_u - 1)] for the input chunk's offsets o --
and Propagate (existing code) runs on it.  Compute on the utterances then
feeds every layer above the Splice the same matrix with the same row count, so
the result must be BIT-IDENTICAL, in the fused and the literal path and in
fusion modes 1 and 2.  For a deeper Splice (nets D, E) a padded single chunk
is not what Propagate's windows are: there each layer of Compute's pass is
checked on its own input, the Splices bit-exactly against numpy indexing with
the per-utterance row counts of the padded pass, the FC layers under
assert_bound at rtol 1e-5 (the bar of the FC tests of test_gpu_nnet2.py)
against the oracle's FC, ReLU exactly, Softmax at the 1e-5 of
test_gpu_nnet2_loss.py.

The log-likelihood epilogue must equal, within 1 ulp of fp32 (correct rounding
plus the double rounding through fp64; nothing measured), the fp64 formula
log(max(P, 1e-20)) - prior_scale * log(prior) applied to the host copy of
Propagate's P and rounded to fp32; fused and literal give the same bits.
"""
import functools

import numpy as np
import pytest

import oracle as O
import nnet2_kernel_cases as T
import nnet2_loss_ref as R
from _pitched import assert_bits, edge_columns, place, stream, sync
from _util import assert_bound, assert_same, dev, host, padded, rng, triple

pytestmark = pytest.mark.gpu

F32 = np.float32
RTOL = 1e-5  # the FC bar of test_gpu_nnet2.py

FC = ("FullyConnectedComponent input-dim={i} output-dim={o} learning-rate=0.02 "
      "param-stddev={s} bias-stddev=0.5 weight-decay=0.0005 momentum=0.9")


def conv_net(d):
    """Net A (d = 5) / net B (d = 8: every splice access 16 bytes)."""
    return "\n".join([
        f"SpliceComponent input-dim={d} left-context=2 right-context=2 const-component-dim=0",
        f"ConvolutionComponent in-height={d} in-width=5 in-channel=1 kernel-height={d} "
        "kernel-width=2 stride=1 group=4 out-height=1 out-width=4 learning-rate=0.02 "
        "param-stddev=0.3 bias-stddev=0.5 weight-decay=0.0005 momentum=0.9",
        "MaxpoolComponent in-height=1 in-width=4 in-channel=4 pool-height-dim=1 "
        "pool-width-dim=2 pool-channel-dim=1",
        "RectifiedLinearComponent dim=8",
        "NormalizeComponent dim=8",
        FC.format(i=8, o=12, s=0.3),
        "SoftmaxComponent dim=12"])


NET_C = "\n".join([
    "SpliceComponent input-dim=6 left-context=1 right-context=1 const-component-dim=2",
    FC.format(i=14, o=9, s=0.3),
    "SoftmaxComponent dim=9"])
NET_D = "\n".join([
    "SpliceComponent input-dim=4 left-context=2 right-context=2 const-component-dim=0",
    FC.format(i=20, o=8, s=0.3),
    "RectifiedLinearComponent dim=8",
    "SpliceComponent input-dim=8 context=-3:0:3 const-component-dim=0",
    FC.format(i=24, o=7, s=0.3),
    "SoftmaxComponent dim=7"])
NET_E = "\n".join([
    "RectifiedLinearComponent dim=4",
    "SpliceComponent input-dim=4 left-context=2 right-context=2 const-component-dim=0",
    FC.format(i=20, o=7, s=0.3),
    "SoftmaxComponent dim=7"])
CONFIGS = {"A": conv_net(5), "B": conv_net(8), "C": NET_C, "D": NET_D, "E": NET_E}


@functools.lru_cache(maxsize=None)
def net_of(name):
    import kcnn
    kcnn.init(0)
    kcnn.set_randn_seed(4100 + ord(name))
    return kcnn.Nnet(CONFIGS[name])


@functools.lru_cache(maxsize=None)
def nnet_config_model():
    import kcnn
    from test_gpu_compute_prob import nnet_config_test_model
    kcnn.init(0)
    return nnet_config_test_model(kcnn)[0]


def utterances(lengths, d, seed):
    r = rng(seed)
    return [r.standard_normal((t, d)).astype(F32) for t in lengths]


def windows(utts, left, right):
    """The matrix Propagate takes: per frame its clamped context window."""
    rows = []
    for x in utts:
        t_max = len(x) - 1
        for t in range(len(x)):
            rows += [x[min(max(t + o, 0), t_max)] for o in range(-left, right + 1)]
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def propagate_reference(name, lengths, seed, literal, fusion):
    """Propagate's output, in the given path and fusion mode, on the windows
    of the utterances; computed once, read by every test of the case."""
    import kcnn
    net = nnet_config_model() if name == "nnet" else net_of(name)
    d = net.components[0].InputDim()
    utts = utterances(lengths, d, seed)
    try:
        kcnn.set_literal_path(literal)
        kcnn.set_fusion(fusion)
        net.Propagate(dev(windows(utts, net.LeftContext(), net.RightContext())))
        out = host(net.Output()).copy()
    finally:
        kcnn.set_literal_path(False)
        kcnn.set_fusion(1)
    out.setflags(write=False)
    return out


def input_dim(name):
    return (nnet_config_model() if name == "nnet" else net_of(name)).components[0].InputDim()


def run_modes(kc, fn):
    """fn() in the fused and the literal path, fusion modes 1 and 2."""
    out = {}
    try:
        for literal in (False, True):
            for fusion in (1, 2):
                kc.set_literal_path(literal)
                kc.set_fusion(fusion)
                out[(literal, fusion)] = fn()
    finally:
        kc.set_literal_path(False)
        kc.set_fusion(1)
    return out


def check_against_propagate(kc, name, lengths, seed, layout="contiguous"):
    net = nnet_config_model() if name == "nnet" else net_of(name)
    utts = utterances(lengths, input_dim(name), seed)
    stacked = np.concatenate(utts)
    x = dev(stacked) if layout == "contiguous" else padded(stacked, layout)
    arg = None if len(lengths) == 1 else list(lengths)
    got = run_modes(kc, lambda: host(net.Compute(x, arg)).copy())
    for mode, y in got.items():
        want = propagate_reference(name, tuple(lengths), seed, *mode)
        assert y.shape == (sum(lengths), want.shape[1])
        assert_same(y, want, f"net {name} {lengths} literal, fusion = {mode}")


@pytest.mark.parametrize("t", [1, 2, 5, 37])  # L = R = 2: T = 1, 2 = L, L + R + 1, 37
@pytest.mark.parametrize("name", ["A", "B"])
def test_single_utterance_is_propagate_on_its_windows(kc, name, t):
    check_against_propagate(kc, name, (t,), 100 + t)


@pytest.mark.parametrize("t", [1, 2, 3, 37])  # L = 1: T = 1, 2, L + R + 1, 37
def test_const_component_tail(kc, t):
    check_against_propagate(kc, "C", (t,), 200 + t)


@pytest.mark.parametrize("lengths", [(1, 7, 23, 2), (5,)])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_batch_is_propagate_on_its_windows(kc, name, lengths):
    check_against_propagate(kc, name, lengths, 300 + len(lengths))


@pytest.mark.parametrize("extra_cols", [3, 4])  # net B: a stride of 11 (scalar), of 12 (16-byte)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_strided_input(kc, name, extra_cols):
    check_against_propagate(kc, name, (1, 7, 23, 2), 304, layout=extra_cols)


def test_many_utterances_many_row_groups(kc):
    """More utterances than a row group holds rows, over several groups: the
    search over the starts."""
    lengths = tuple(int(t) for t in rng(7).integers(1, 9, size=150))
    check_against_propagate(kc, "B", lengths, 305)


@pytest.mark.parametrize("d", [205, 820])  # 1025 columns (scalar), 4100 (16-byte accesses)
def test_more_row_groups_than_blocks(kc, d):
    """Rows this wide make every output row a group of its own, and 8300 rows
    are more groups than the grid has blocks (8192): the blocks' stride over
    the groups, which no smaller shape reaches.  A Splice alone, against numpy
    indexing."""
    net = kc.Nnet(f"SpliceComponent input-dim={d} left-context=2 right-context=2 "
                  "const-component-dim=0")
    lengths = (1, 4000, 4299)
    x = rng(306).standard_normal((sum(lengths), d)).astype(F32)
    want, start = [], 0
    for t in lengths:
        idx = np.clip(np.arange(t)[:, None] + np.arange(-2, 3)[None, :], 0, t - 1)
        want.append(x[start + idx].reshape(t, 5 * d))
        start += t
    assert_same(host(net.Compute(dev(x), list(lengths))), np.concatenate(want), f"dim {d}")


def test_nnet_config_two_utterances(kc):
    check_against_propagate(kc, "nnet", (3, 8), 400)


def test_contexts(kc):
    assert (net_of("A").LeftContext(), net_of("A").RightContext()) == (2, 2)
    assert (net_of("D").LeftContext(), net_of("D").RightContext()) == (5, 5)
    assert (net_of("E").LeftContext(), net_of("E").RightContext()) == (2, 2)
    m = nnet_config_model()
    assert (m.LeftContext(), m.RightContext()) == (10, 10)


# ---- pad_input=False ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_unpadded(kc, name):
    net = net_of(name)
    left, right = net.LeftContext(), net.RightContext()
    span = left + right
    d = input_dim(name)
    # T = L + R + 1: one row, Propagate on the utterance itself as one window
    (x,) = utterances((span + 1,), d, 500)

    def propagate(win):
        net.Propagate(dev(win))
        return host(net.Output()).copy()
    got = run_modes(kc, lambda: (propagate(x),
                                 host(net.Compute(dev(x), pad_input=False)).copy()))
    for mode, (want, y) in got.items():
        assert y.shape == (1, want.shape[1])
        assert_same(y, want, f"net {name} unpadded {mode}")
    # a batch [L + R + 1, L + R + 4]: the windows are the frames themselves
    utts = utterances((span + 1, span + 4), d, 501)
    win = np.concatenate([u[t:t + span + 1] for u in utts for t in range(len(u) - span)])
    xs = dev(np.concatenate(utts))
    got = run_modes(kc, lambda: (propagate(win), host(
        net.Compute(xs, [span + 1, span + 4], pad_input=False)).copy()))
    for mode, (want, y) in got.items():
        assert y.shape == (5, want.shape[1])
        assert_same(y, want, f"net {name} unpadded batch {mode}")


def test_unpadded_short_utterance_is_refused(kc):
    net = net_of("A")
    (x,) = utterances((5,), 5, 502)
    before = host(net.Compute(dev(x))).copy()
    with pytest.raises(kc.KcnnError, match="at least 5"):
        net.Compute(dev(x[:4]), pad_input=False)  # T = L + R
    with pytest.raises(kc.KcnnError, match="at least 5"):
        net.Compute(dev(np.concatenate([x, x[:4]])), [5, 4], pad_input=False)
    assert_same(host(net.Output()), before, "the last result after a refused call")


# ---- deeper splices: each layer of the padded single-chunk pass ---------------------
def splice_rows(x_utts, context, const_dim=0):
    """SpliceComponent on whole utterances by indexing: output row t of an
    utterance of n rows reads rows t + c - context[0]."""
    out = []
    span = context[-1] - context[0]
    for x in x_utts:
        n_out = len(x) - span
        d = x.shape[1] - const_dim
        rows = [np.concatenate([x[t + c - context[0], :d] for c in context] + [x[t, d:]])
                for t in range(n_out)]
        out.append(np.stack(rows))
    return out


def const_dim(comp):
    """const-component-dim of a SpliceComponent, from its dimensions."""
    n = len(comp.Context())
    return 0 if n == 1 else (n * comp.InputDim() - comp.OutputDim()) // (n - 1)


def split(a, counts):
    assert a.shape[0] == sum(counts), (a.shape, counts)
    return np.split(a, np.cumsum(counts)[:-1])


def clamp_pad(utts, left, right):
    return [x[np.clip(np.arange(-left, len(x) + right), 0, len(x) - 1)] for x in utts]


def check_layers(kc, name, lengths, pad_input, seed):
    net = net_of(name)
    left, right = net.LeftContext(), net.RightContext()
    utts = utterances(lengths, input_dim(name), seed)
    out_frames = [t if pad_input else t - left - right for t in lengths]
    y = net.Compute(dev(np.concatenate(utts)), list(lengths), pad_input=pad_input)
    assert y.shape[0] == sum(out_frames)
    contexts = [list(c.Context()) for c in net.components]
    # rows an utterance has at each activation: its result's plus the context
    # of the components above
    ext = [0]
    for ctx in reversed(contexts):
        ext.insert(0, ext[0] + ctx[-1] - ctx[0])
    acts = [host(net.Output(i)).copy() for i in range(net.NumComponents())]
    if pad_input and contexts[0] == [0]:
        # the clamped frames laid out for a row-wise first component
        assert_same(host(net.Output(-1)), np.concatenate(clamp_pad(utts, left, right)), "layout")
    cur = clamp_pad(utts, left, right) if pad_input else utts
    assert [len(c) for c in cur] == [n + ext[0] for n in out_frames]
    for i, comp in enumerate(net.components):
        counts = [n + ext[i + 1] for n in out_frames]
        got = acts[i]
        kind = comp.Type()
        x = np.concatenate(cur)
        if kind == "SpliceComponent":
            assert_same(got, np.concatenate(splice_rows(cur, contexts[i], const_dim(comp))),
                        f"{name} Splice {i}")
        elif kind == "RectifiedLinearComponent":
            assert_same(got, np.where(x < 0, F32(0), x), f"{name} ReLU {i}")
        elif kind == "FullyConnectedComponent":
            of = O.FC(comp.InputDim(), comp.OutputDim())
            of.W, of.b = host(comp.LinearParams()), host(comp.BiasParams())
            _, t, s = triple(lambda: of.propagate(x))
            assert_bound(got, t, s, rtol=RTOL, what=f"{name} FC {i}")
        else:
            assert kind == "SoftmaxComponent"
            t = R.softmax_prop64(x)
            assert (np.abs(got - t) <= RTOL * np.abs(t)).all(), f"{name} Softmax {i}"
        # the next layer is checked on the device's own activation
        cur = split(got, counts)
    assert_same(host(y), acts[-1], "the result is the last output")


@pytest.mark.parametrize("pad_input", [True, False])
@pytest.mark.parametrize("name", ["D", "E"])
def test_deeper_splice_layers(kc, name, pad_input):
    span = net_of(name).LeftContext() + net_of(name).RightContext()
    lengths = (1, 7, 23, 2) if pad_input else (span + 1, span + 4)
    check_layers(kc, name, lengths, pad_input, 600)
    check_layers(kc, name, (1,) if pad_input else (span + 6,), pad_input, 601)


def result_error_scale(net, lengths):
    """From the activations the last Compute (padded, on utterances of
    `lengths`) left: S such that two results that each hold the FC bar differ
    by at most RTOL * S.  An FC's output is within RTOL * S_fc of exact (S_fc
    the sum of |terms|, the oracle's third mode) and passes an input error E
    on as E |W|^T; a Splice copies E as it copies rows; ReLU does not grow it;
    through the Softmax |dP| <= 2 P max|dx|; and two such results differ by
    twice that."""
    contexts = [list(c.Context()) for c in net.components]
    ext = [0]
    for ctx in reversed(contexts):
        ext.insert(0, ext[0] + ctx[-1] - ctx[0])
    err = None  # the network input is exact
    for i, comp in enumerate(net.components):
        kind = comp.Type()
        x = host(net.Output(i - 1)).copy()
        if err is None:
            err = np.zeros((sum(lengths) + len(lengths) * ext[0], x.shape[1]))
        if kind == "SpliceComponent":
            err = np.concatenate(splice_rows(split(err, [t + ext[i] for t in lengths]),
                                             contexts[i], const_dim(comp)))
        elif kind == "FullyConnectedComponent":
            of = O.FC(comp.InputDim(), comp.OutputDim())
            of.W, of.b = host(comp.LinearParams()), host(comp.BiasParams())
            _, _, s = triple(lambda: of.propagate(x))
            err = s.astype(np.float64) + err @ np.abs(of.W.astype(np.float64)).T
        elif kind == "SoftmaxComponent":
            p = host(net.Output(i)).astype(np.float64)
            err = 2.0 * p * err.max(axis=1, keepdims=True)
        else:
            assert kind == "RectifiedLinearComponent", kind
    return 2.0 * err


@pytest.mark.parametrize("name", ["C", "D"])
def test_batch_against_single(kc, name):
    """Compute on [7, 23] against the two single-utterance calls, under
    assert_bound alone at the FC bar: the FC GEMMs scale their operands per
    column of the whole input matrix, so an utterance's rows are rounded
    differently beside another utterance than alone, and the bits differ.
    The error scale is result_error_scale's."""
    net = net_of(name)
    utts = utterances((7, 23), input_dim(name), 700)
    single = np.concatenate([host(net.Compute(dev(u))).copy() for u in utts])
    both = host(net.Compute(dev(np.concatenate(utts)), [7, 23])).copy()
    scale = result_error_scale(net, (7, 23))
    assert both.shape == single.shape == scale.shape
    print(f"net {name}: worst |batch - single| / S = "
          f"{(np.abs(both.astype(np.float64) - single) / scale).max():.3e}")
    assert_bound(both, single, scale, rtol=RTOL, what=f"net {name}")


# ---- the log-likelihood epilogue ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def softmax_net(cols):
    import kcnn
    kcnn.init(0)
    return kcnn.Nnet(f"SoftmaxComponent dim={cols}")


def expected_loglikes(p, priors=None, prior_scale=1.0):
    with np.errstate(all="ignore"):
        floored = np.where(p < F32(1e-20), F32(1e-20), p).astype(np.float64)
        ll = np.log(floored)
        if priors is not None:
            ll = ll - np.float64(prior_scale) * np.log(np.asarray(priors, F32).astype(np.float64))
        return ll.astype(F32)


def assert_within_one_ulp(got, want, what):
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), f"{what}: NaNs differ"
    g, w = got[~nan], want[~nan]
    # neighbours of the expected fp32 value
    lo, hi = np.nextafter(w, F32(-np.inf)), np.nextafter(w, F32(np.inf))
    bad = (g < lo) | (g > hi)
    print(f"{what}: {int((g != w).sum())} of {g.size} differ from the rounded fp64 value")
    assert not bad.any(), f"{what}: {bad.sum()} elements past 1 ulp"


def both_paths(kc, net, x, **kw):
    got = {}
    try:
        for literal in (False, True):
            kc.set_literal_path(literal)
            got[literal] = host(net.Compute(x, **kw)).copy()
    finally:
        kc.set_literal_path(False)
    assert_same(got[False], got[True], "fused against literal")
    return got[False]


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", [12, 13, 3454])
def test_loglikes(kc, rows, cols):
    r = rng(800 + cols + rows)
    logits = (r.standard_normal((rows, cols)) * 3).astype(F32)
    priors = (r.random(cols) + 0.01).astype(F32)
    net = softmax_net(cols)
    x = dev(logits)
    net.Propagate(x)
    p = host(net.Output()).copy()
    assert_same(host(net.Compute(x)), p, "neither log nor priors: P itself")
    for kw in ({"priors": priors}, {"priors": priors, "prior_scale": 0.5}, {}):
        got = both_paths(kc, net, x, apply_log=True, **kw)
        assert_within_one_ulp(got, expected_loglikes(p, **kw), f"{rows}x{cols} {sorted(kw)}")


@pytest.mark.parametrize("cols", [13, 3454])
def test_loglikes_special_rows(kc, cols):
    r = rng(810 + cols)
    logits = (r.standard_normal((5, cols)) * 3).astype(F32)
    logits[1, 3] = np.nan
    logits[3, 7] = -np.inf
    priors = (r.random(cols) + 0.01).astype(F32)
    net = softmax_net(cols)
    x = dev(logits)
    net.Propagate(x)
    p = host(net.Output()).copy()
    assert np.isnan(p[1]).all() and p[3, 7] == F32(1e-20)
    got = both_paths(kc, net, x, apply_log=True, priors=priors)
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2, 3, 4]]).any()
    assert_within_one_ulp(got, expected_loglikes(p, priors), f"special {cols}")
    want = F32(np.log(np.float64(F32(1e-20))) - np.log(np.float64(priors[7])))
    assert abs(float(got[3, 7]) - float(want)) <= abs(float(np.spacing(want)))


@pytest.mark.parametrize("case", T.select("kn_softmax_loglikes"), ids=T.name_of)
def test_softmax_loglikes_layouts(kc, case):
    """kn_softmax_loglikes directly, on pitched operands with sentinels at the
    layouts of tests/nnet2_kernel_cases.py (every access width at every count of
    values a lane holds; tests/test_nnet2_routes.py pins the kernel).  The
    expected P: kn_softmax_prop into an output laid out as `out`
    (nnet-kernels.h); with more than one row, a -inf logit in row 0's edge
    columns (in an only row it would hide a dropped last column)."""
    import torch
    KN = T.bind(kc)
    rows, cols = case["rows"], case["cols"]
    r = rng(820 + cols + rows)
    logits = (r.standard_normal((rows, cols)) * 3).astype(F32)
    if rows > 1:
        logits[0, edge_columns(cols)] = -np.inf
    priors = (r.random(cols) + 0.01).astype(F32)
    offset = torch.from_numpy(np.log(priors.astype(np.float64))).cuda()
    X, Pm = place(kc, case["ops"][0], logits), place(kc, case["ops"][1])
    assert KN.kn_softmax_prop(X.ptr, X.dim, Pm.ptr, Pm.dim, stream()) == 0
    sync()
    p = Pm.get()
    assert rows == 1 or (p[0, edge_columns(cols)] == F32(1e-20)).all()
    for off, pri in ((offset, priors), (None, None)):
        Y = place(kc, case["ops"][1])
        assert KN.kn_softmax_loglikes(X.ptr, X.dim, Y.ptr, Y.dim,
                                      off.data_ptr() if off is not None else None, stream()) == 0
        sync()
        assert_within_one_ulp(Y.get(), expected_loglikes(p, pri), case["name"])
    assert_bits(X.get(), logits, "the logits")


def test_loglikes_of_a_network_without_softmax(kc):
    """The element-wise kernel alone: the last component is not a Softmax, and
    a value under the floor is floored."""
    net = kc.Nnet("RectifiedLinearComponent dim=13")
    x = (rng(820).random((5, 13)) + 0.1).astype(F32)
    x[2, 4] = 0.0
    x[4, 1] = -1.0
    priors = (rng(821).random(13) + 0.01).astype(F32)
    p = np.where(x < 0, F32(0), x)
    got = both_paths(kc, net, dev(x), apply_log=True, priors=priors, prior_scale=0.5)
    assert_within_one_ulp(got, expected_loglikes(p, priors, 0.5), "ReLU network")


def test_refused_priors_run_nothing(kc):
    net = softmax_net(12)
    x = dev((rng(830).standard_normal((5, 12)) * 3).astype(F32))
    good = np.full(12, 0.25, F32)
    before = host(net.Compute(x, apply_log=True, priors=good)).copy()
    view = net.Compute(x, apply_log=True, priors=good)
    for at, bad in ((3, 0.0), (3, -0.5), (3, np.nan), (3, np.inf)):
        pr = good.copy()
        pr[at] = bad
        with pytest.raises(kc.KcnnError, match="prior"):
            net.Compute(x, apply_log=True, priors=pr)
    for n in (11, 13):
        with pytest.raises(kc.KcnnError, match="priors for 12"):
            net.Compute(x, apply_log=True, priors=np.full(n, 0.25, F32))
    with pytest.raises(kc.KcnnError, match="apply_log"):
        net.Compute(x, priors=good)
    assert_same(host(view), before, "the last result after the refused calls")


def test_refused_lengths_run_nothing(kc):
    net = net_of("A")
    (x,) = utterances((9,), 5, 840)
    before = host(net.Compute(dev(x))).copy()
    view = net.Compute(dev(x))
    for lengths in ([4, 4], [0, 9], [-1, 10], [], [9, 1]):
        with pytest.raises(kc.KcnnError):
            net.Compute(dev(x), lengths)
    with pytest.raises(kc.KcnnError):
        net.Compute(dev(np.zeros((9, 4), F32)))  # 4 columns for a 5-column network
    assert_same(host(view), before, "the last result after the refused calls")


# ---- state -----------------------------------------------------------------------------
def bits_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def snapshot(net):
    """Every parameter and PrevGrad (device), every NonlinearComponent statistic."""
    params, stats = [], []
    for c in net.components:
        if c.NumGradientParams() > 0:
            params += [c.GetParam(w).clone() for w in (0, 1, 2)]
        elif c.Type() in ("RectifiedLinearComponent", "SoftmaxComponent", "NormalizeComponent"):
            vs, ds, cnt = c.NonlinearStats()
            stats.append((vs.copy(), ds.copy(), cnt))
    return params, stats


def assert_unchanged(before, after):
    assert len(before[0]) == len(after[0])
    for a, b in zip(before[0], after[0]):
        assert bits_equal(a, b), "a parameter changed"
    assert len(before[1]) == len(after[1])
    for (v0, d0, c0), (v1, d1, c1) in zip(before[1], after[1]):
        np.testing.assert_array_equal(v0, v1)
        np.testing.assert_array_equal(d0, d1)
        assert c0 == c1


@pytest.mark.parametrize("literal", [False, True])
def test_state_after_compute(kc, literal):
    kc.set_randn_seed(900)
    net = kc.Nnet(CONFIGS["A"])
    utts = utterances((7, 3), 5, 901)
    win = dev(windows(utts, 2, 2))
    labels = [(i, i % 12, 1.0) for i in range(10)]
    net.Propagate(win)  # a training step first: statistics and PrevGrad are not zero
    net.BackpropXent(labels)
    net.ObjfTotal(reset=True)
    before = snapshot(net)
    x = dev(np.concatenate(utts))
    kc.set_literal_path(literal)
    try:
        y = host(net.Compute(x, [7, 3], apply_log=True, priors=np.full(12, 0.1, F32))).copy()
        assert y.shape == (10, 12)
        dy = dev(np.zeros((10, 12), F32))
        for call in (lambda: net.BackpropXent(labels), lambda: net.Backprop(dy),
                     lambda: net.BackpropComponent(net.NumComponents() - 1, dy)):
            with pytest.raises(kc.KcnnError, match="propagate first"):
                call()
        # the last output is there on request, the Softmax not having run
        net2 = net.Copy()
        net2.Propagate(win)
        assert_same(host(net.Output()), host(net2.Output()), "P after Compute")
    finally:
        kc.set_literal_path(False)
    assert_unchanged(before, snapshot(net))
    assert net.ObjfTotal() == (0.0, 0.0) and net.ProbTotal() == (0.0, 0.0, 0.0)
    # after a Propagate the network trains again
    net.Propagate(win)
    net.BackpropXent(labels)
    assert net.ObjfTotal()[1] == 10
    after = snapshot(net)
    assert not all(bits_equal(a, b) for a, b in zip(before[0], after[0]))
