"""Nnet.Compute(share_time=True): the leading Splice -> {Convolution | Maxpool
| ReLU}... components run once per time step (time maps) instead of once per
window, on the GPU.

1. Each level on its own input: TimeMap(l) at its valid rows against
   TimeMap(l - 1).  A convolution against fp64 under assert_bound(rtol=1e-5)
   with S = sum |terms| + |b| (the FC bar: these are the same GEMMs); pool and
   ReLU bit-exact against a numpy fp32 restatement of the reference's fold;
   level 0 bit-exact against the (clamped) frames; Output(p - 1) bit-exact
   against numpy indexing of the last map.
2. Against Compute: Output(p - 1) of the two passes differs by at most 2 E, E
   the per-layer bar propagated in fp64 (E' = |W| (*) E + 1e-5 S through a
   convolution, the window maximum of E through a pool, unchanged through a
   ReLU): derived from the bar, not measured.
3. Integer data (inputs in {-2..2}, weights in {-1, 0, 1} with at most 4
   non-zeros a filter, integer biases, every activation below 2^11, asserted
   on the reference): every operand is one f16 / bf16 part and every sum exact
   in any order, so Output(p - 1) of both passes equals the oracle's window
   pass bit for bit and the final results are bit-identical.
4. Dynamic range: an utterance scaled by 1e6 beside one scaled by 1e-6.
5. Fallbacks and state.
6. nnet.config's test model: prefix 14, check 1 on all 13 levels.

Unpadded, an utterance of T <= L + R frames is an error by Compute's contract,
so the unpadded cases run the listed lengths as RESULT frames (T + L + R input
frames)."""
import functools

import numpy as np
import pytest

import oracle as O
from _util import assert_bound, assert_same, dev, host, padded, rng
from test_gpu_compute import (CONFIGS, FC, net_of, nnet_config_model, utterances, windows)

pytestmark = pytest.mark.gpu

F32 = np.float32
RTOL = 1e-5  # the FC bar of test_gpu_nnet2.py
CONV = ("ConvolutionComponent in-height={h} in-width={w} in-channel={c} kernel-height={h} "
        "kernel-width={kw} stride=1 group={g} out-height=1 out-width={ow} learning-rate=0.02 "
        "param-stddev=0.3 bias-stddev=0.5 weight-decay=0.0005 momentum=0.9")
POOL = ("MaxpoolComponent in-height=1 in-width={w} in-channel={c} pool-height-dim=1 "
        "pool-width-dim={pw} pool-channel-dim={pc}")


def shrunken(channel_pool):
    """nnet.config shrunken: Splice d = 8, L = R = 5; conv kw 4 -> 32, ReLU;
    conv kw 3 -> 32; pool 1 x 2 (channel_pool: 1 x 1 x 4); ReLU; conv kw 2 ->
    64 (at dilation 2 after the 1 x 2 pool); ReLU; FC; Softmax."""
    pw, pc = (1, 4) if channel_pool else (2, 1)
    w, c = 6 // pw, 32 // pc
    return "\n".join([
        "SpliceComponent input-dim=8 left-context=5 right-context=5 const-component-dim=0",
        CONV.format(h=8, w=11, c=1, kw=4, g=32, ow=8),
        "RectifiedLinearComponent dim=256",
        CONV.format(h=1, w=8, c=32, kw=3, g=32, ow=6),
        POOL.format(w=6, c=32, pw=pw, pc=pc),
        f"RectifiedLinearComponent dim={w * c}",
        CONV.format(h=1, w=w, c=c, kw=2, g=64, ow=w - 1),
        f"RectifiedLinearComponent dim={(w - 1) * 64}",
        FC.format(i=(w - 1) * 64, o=10, s=0.3),
        "SoftmaxComponent dim=10"])


SHARED_CONFIGS = {"S": shrunken(False), "P": shrunken(True)}
PREFIX = {"A": 4, "B": 4, "S": 8, "P": 8}


@functools.lru_cache(maxsize=None)
def shared_net(name):
    if name in ("A", "B"):
        return net_of(name)
    import kcnn
    kcnn.init(0)
    kcnn.set_randn_seed(5100 + ord(name))
    return kcnn.Nnet(SHARED_CONFIGS[name])


class Geometry:
    """The rows of one pass: utterance u has its first row base[u] in every
    map and gives frames[u] result rows from result row start[u]."""

    def __init__(self, net, lengths, pad):
        self.left, self.right = net.LeftContext(), net.RightContext()
        self.context = self.left + self.right
        self.lengths, self.pad = list(lengths), pad
        self.frames = [t if pad else t - self.context for t in lengths]
        rows = [f + self.context for f in self.frames]
        self.base = [int(b) for b in np.cumsum([0] + rows[:-1])]
        self.start = [int(s) for s in np.cumsum([0] + self.frames[:-1])]
        self.input_rows, self.total = sum(rows), sum(self.frames)

    def valid(self, n, delta):
        """The rows of a level (n positions at dilation delta) that windows read."""
        return np.concatenate([np.arange(b, b + f + delta * (n - 1))
                               for b, f in zip(self.base, self.frames)])

    def level0(self, utts):
        if not self.pad:
            return np.concatenate(utts)
        return np.concatenate([x[np.clip(np.arange(-self.left, len(x) + self.right), 0,
                                         len(x) - 1)] for x in utts])

    def gather(self, m, n, delta):
        """out[row(u, t)][k + c n] = m[base_u + t + delta k][c]"""
        out = np.empty((self.total, m.shape[1] * n), m.dtype)
        for b, s, f in zip(self.base, self.start, self.frames):
            for k in range(n):
                out[s:s + f, k::n] = m[b + delta * k:b + delta * k + f]
        return out


def taps(comp, below_kind, below_width):
    """The weight block of each tap of a time-map convolution, its bias."""
    w, b = host(comp.LinearParams()), host(comp.BiasParams())
    kw = w.shape[0] // below_width
    if below_kind == "SpliceComponent":
        return [w[d * below_width:(d + 1) * below_width] for d in range(kw)], b
    return [w[d::kw] for d in range(kw)], b


def line_args(line):
    """The integer arguments of a config line."""
    out = {}
    for tok in line.split():
        key, _, val = tok.partition("=")
        if val.lstrip("-").isdigit():
            out[key] = int(val)
    return out


def config_lines(name):
    """The config lines of a net of this file, of test_gpu_compute.py, or of
    tests/golden/nnet.config ("nnet")."""
    if name == "nnet":
        import os
        golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        text = open(os.path.join(golden, "nnet.config")).read()
    else:
        text = SHARED_CONFIGS[name] if name in SHARED_CONFIGS else CONFIGS[name]
    return [ln for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]


def fold(a, rows, delta, pw, pc):
    """The reference's Maxpool fold (start -1e20f, replace when v < x) over
    c < pc (outer), w < pw (inner) of a[rows + delta w][oc pc + c], in fp32."""
    v = np.full((len(rows), a.shape[1] // pc), F32(-1e20), F32)
    for c in range(pc):
        for w in range(pw):
            x = a[rows + delta * w][:, c::pc]
            v = np.where(v < x, x, v)
    return v


def read_maps(net):
    p = net.TimeSharedPrefix()
    maps = []
    for lvl in range(p):
        view, c, n, d = net.TimeMap(lvl)
        maps.append((host(view).copy(), c, n, d))
    return maps


def check_levels(name, net, prefix, utts, lengths, pad, x, what, against_compute=True):
    """Checks 1 and (against_compute) 2 for one pass of the net whose config is
    config_lines(name); returns (shared result, Compute's result or None)."""
    args = [line_args(ln) for ln in config_lines(name)]
    geo = Geometry(net, lengths, pad)
    arg = list(lengths)
    assert net.TimeSharedPrefix() == prefix
    y = host(net.Compute(x, arg, pad_input=pad, share_time=True)).copy()
    maps = read_maps(net)
    top = host(net.Output(prefix - 1)).copy()
    assert len(maps) == prefix and y.shape[0] == geo.total
    m0, c0, n0, d0 = maps[0]
    assert (c0, n0, d0) == (1, geo.context + 1, 1) and m0.shape[0] == geo.input_rows
    assert_same(m0, geo.level0(utts), f"{what}: level 0")
    err = np.zeros(m0.shape)  # the bar E of each level, at every row (used at valid rows)
    kinds = [c.Type() for c in net.components]
    for lvl in range(1, prefix):
        comp = net.components[lvl]
        a, _, n_in, d_in = maps[lvl - 1]
        got, c, n, d = maps[lvl]
        assert got.shape[1] == c
        rows = geo.valid(n, d)
        assert rows.max() < got.shape[0], (lvl, rows.max(), got.shape)
        e_out = np.zeros(got.shape)
        if kinds[lvl] == "ConvolutionComponent":
            ws, b = taps(comp, kinds[lvl - 1], a.shape[1])
            assert (n, d) == (n_in - len(ws) + 1, d_in)
            a64 = a.astype(np.float64)
            t = np.tile(b.astype(np.float64), (len(rows), 1))
            s = np.abs(t)
            e = np.zeros_like(t)
            for k, w in enumerate(ws):
                w64 = w.astype(np.float64)
                t += a64[rows + d_in * k] @ w64
                s += np.abs(a64[rows + d_in * k]) @ np.abs(w64)
                e += err[rows + d_in * k] @ np.abs(w64)
            worst = (np.abs(got[rows] - t) / np.maximum(s, 1e-30)).max()
            print(f"{what}: level {lvl} conv {a.shape[1]} x {len(ws)} -> {c}: worst err / S = "
                  f"{worst:.3e}")
            assert_bound(got[rows], t, s, rtol=RTOL, what=f"{what}: level {lvl} convolution")
            e_out[rows] = e + RTOL * s
        elif kinds[lvl] == "MaxpoolComponent":
            pw, pc = args[lvl]["pool-width-dim"], args[lvl]["pool-channel-dim"]
            assert (c, n, d) == (a.shape[1] // pc, n_in // pw, d_in * pw)
            assert_same(got[rows], fold(a, rows, d_in, pw, pc), f"{what}: level {lvl} pool")
            e_out[rows] = np.max([err[rows + d_in * w][:, ch::pc] for ch in range(pc)
                                  for w in range(pw)], axis=0)
        else:
            assert kinds[lvl] == "RectifiedLinearComponent" and (n, d) == (n_in, d_in)
            assert_same(got[rows], np.where(a[rows] < 0, F32(0), a[rows]),
                        f"{what}: level {lvl} ReLU")
            e_out[rows] = err[rows]
        err = e_out
    last, c, n, d = maps[-1]
    assert top.shape == (geo.total, c * n)
    assert_same(top, geo.gather(last, n, d), f"{what}: Output({prefix - 1}) is the gathered map")
    if not against_compute:
        return y, None
    # check 2: Compute's own Output(p - 1), each within E of the truth
    y_own = host(net.Compute(x, arg, pad_input=pad)).copy()
    top_own = host(net.Output(prefix - 1)).copy()
    bar = 2.0 * geo.gather(err, n, d)
    diff = np.abs(top.astype(np.float64) - top_own)
    print(f"{what}: worst |shared - Compute| / 2E = "
          f"{(diff / np.maximum(bar, 1e-300)).max():.3e}")
    assert (diff <= bar).all(), f"{what}: {(diff > bar).sum()} elements of Output differ by more than 2 E"
    assert y.shape == y_own.shape
    return y, y_own


LENGTHS = {"A": (1, 2, 5, 37), "B": (1, 2, 5, 37), "S": (1, 2, 5, 11, 37), "P": (1, 2, 5, 11, 37)}
CASES = [(name, (t,)) for name in "ABSP" for t in LENGTHS[name]] + \
        [(name, (1, 37, 5, 300)) for name in "ABSP"]


def case_input(name, frames, pad, seed):
    net = shared_net(name)
    context = net.LeftContext() + net.RightContext()
    lengths = tuple(frames) if pad else tuple(f + context for f in frames)
    utts = utterances(lengths, net.components[0].InputDim(), seed)
    return net, lengths, utts


@pytest.mark.parametrize("pad", [True, False], ids=["padded", "unpadded"])
@pytest.mark.parametrize("name, frames", CASES, ids=[f"{n}-{'+'.join(map(str, f))}"
                                                     for n, f in CASES])
def test_levels_and_against_compute(kc, name, frames, pad):
    net, lengths, utts = case_input(name, frames, pad, 1000 + sum(frames))
    check_levels(name, net, PREFIX[name], utts, lengths, pad, dev(np.concatenate(utts)),
                 f"net {name} {lengths}")


# ---- 3. exact arithmetic ---------------------------------------------------------------
INPUT_RANGE = 2  # inputs in {-2 .. 2}


@functools.lru_cache(maxsize=None)
def integer_net(name):
    """The net with integer parameters in its prefix: weights in {-1, 0, 1},
    at most 4 non-zeros a filter, biases in {-2 .. 2}."""
    import torch
    import kcnn
    kcnn.init(0)
    kcnn.set_randn_seed(5200 + ord(name))
    net = kcnn.Nnet(CONFIGS[name] if name in ("A", "B") else SHARED_CONFIGS[name])
    r = rng(5300 + ord(name))
    for comp in net.components[:PREFIX[name]]:
        if comp.Type() != "ConvolutionComponent":
            continue
        k, g = comp.ParamDim(0)
        w = np.zeros((k, g), F32)
        for col in range(g):
            at = r.choice(k, size=min(4, k), replace=False)
            w[at, col] = r.choice([-1.0, 1.0], size=len(at))
        comp.SetParam(0, torch.from_numpy(w).cuda())
        comp.SetParam(1, torch.from_numpy(r.integers(-2, 3, size=g).astype(F32)).cuda())
    return net


def oracle_prefix(name, net, prefix, win):
    """The window pass of components 1 .. prefix - 1 by the oracle, in fp32;
    also the largest |activation|."""
    x, biggest = win, float(np.abs(win).max())
    lines = config_lines(name)
    for i in range(1, prefix):
        comp, a = net.components[i], line_args(lines[i])
        kind = comp.Type()
        if kind == "ConvolutionComponent":
            oc = O.Conv(a["in-height"], a["in-width"], a["in-channel"], a["kernel-height"],
                        a["kernel-width"], a["group"])
            oc.W, oc.b = host(comp.LinearParams()), host(comp.BiasParams())
            x = oc.propagate(x)
        elif kind == "MaxpoolComponent":
            x = O.Pool(a["in-height"], a["in-width"], a["in-channel"], a["pool-height-dim"],
                       a["pool-width-dim"], a["pool-channel-dim"]).propagate(x)
        else:
            x = np.where(x < 0, F32(0), x)
        biggest = max(biggest, float(np.abs(x).max()))
    return x, biggest


@pytest.mark.parametrize("pad", [True, False], ids=["padded", "unpadded"])
@pytest.mark.parametrize("name", ["A", "B", "S", "P"])
def test_integer_data_is_exact_and_the_result_bit_identical(kc, name, pad):
    net = integer_net(name)
    prefix = PREFIX[name]
    left, right = net.LeftContext(), net.RightContext()
    frames = (1, 37, 5, 300)
    lengths = frames if pad else tuple(f + left + right for f in frames)
    d = net.components[0].InputDim()
    r = rng(5400 + ord(name))
    utts = [r.integers(-INPUT_RANGE, INPUT_RANGE + 1, size=(t, d)).astype(F32) for t in lengths]
    if pad:
        win = windows(utts, left, right)
    else:
        span = left + right
        win = np.concatenate([u[t:t + span + 1] for u in utts for t in range(len(u) - span)])
    want, biggest = oracle_prefix(name, net, prefix, np.ascontiguousarray(win.reshape(sum(frames), -1)))
    assert biggest < 2 ** 11, biggest
    assert (want == np.round(want)).all()
    x = dev(np.concatenate(utts))
    priors = (rng(5500).random(net.components[-1].OutputDim()) + 0.01).astype(F32)
    for kw in ({}, {"apply_log": True}, {"apply_log": True, "priors": priors, "prior_scale": 0.5}):
        y = host(net.Compute(x, list(lengths), pad_input=pad, share_time=True, **kw)).copy()
        top = host(net.Output(prefix - 1)).copy()
        y_own = host(net.Compute(x, list(lengths), pad_input=pad, **kw)).copy()
        top_own = host(net.Output(prefix - 1)).copy()
        print(f"net {name}: shared differs from the integers in {(top != want).sum()} of "
              f"{want.size}, Compute in {(top_own != want).sum()}; largest |activation| {biggest}")
        assert_same(top, want, f"net {name}: shared Output({prefix - 1}) against the integers")
        assert_same(top_own, want, f"net {name}: Compute's Output({prefix - 1})")
        assert_same(y, y_own, f"net {name}: the result {sorted(kw)}")


# ---- 4. dynamic range -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "S"])
def test_dynamic_range(kc, name):
    """One utterance scaled by 1e6 beside one scaled by 1e-6: every level of
    each still meets check 1 (the GEMMs scale their operands per row); the
    rows that straddle the two are read by nothing."""
    net = shared_net(name)
    lengths = (23, 19)
    utts = utterances(lengths, net.components[0].InputDim(), 1400)
    utts = [utts[0] * F32(1e6), utts[1] * F32(1e-6)]
    check_levels(name, net, PREFIX[name], utts, lengths, True, dev(np.concatenate(utts)),
                 f"net {name} scaled", against_compute=False)


# ---- 5. fallbacks and state ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["C", "D", "E"])
def test_declined_networks_give_computes_bits(kc, name):
    net = net_of(name)
    assert net.TimeSharedPrefix() == 0
    lengths = (1, 7, 23, 2)
    utts = utterances(lengths, net.components[0].InputDim(), 1500)
    x = dev(np.concatenate(utts))
    own = host(net.Compute(x, list(lengths))).copy()
    assert_same(host(net.Compute(x, list(lengths), share_time=True)), own, f"net {name}")
    with pytest.raises(kc.KcnnError, match="kcnn_nnet_compute_shared"):
        net.TimeMap(0)


def test_prefixes(kc):
    import kcnn
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert nnet_config_model().TimeSharedPrefix() == 14
    kcnn.set_randn_seed(1501)
    assert kcnn.Nnet(open(os.path.join(golden, "train_conv.config")).read()).TimeSharedPrefix() == 4
    assert [net_of(n).TimeSharedPrefix() for n in "ABCDE"] == [4, 4, 0, 0, 0]
    assert [shared_net(n).TimeSharedPrefix() for n in "SP"] == [8, 8]


def test_literal_path_gives_computes_bits(kc):
    net = shared_net("S")
    lengths = (7, 23)
    utts = utterances(lengths, 8, 1510)
    x = dev(np.concatenate(utts))
    try:
        kc.set_literal_path(True)
        assert net.TimeSharedPrefix() == 0
        own = host(net.Compute(x, list(lengths))).copy()
        assert_same(host(net.Compute(x, list(lengths), share_time=True)), own, "literal")
    finally:
        kc.set_literal_path(False)
    assert net.TimeSharedPrefix() == 8


@pytest.mark.parametrize("extra_cols", [3, 4])  # a stride of 11 (scalar), of 12 (16-byte)
@pytest.mark.parametrize("pad", [True, False], ids=["padded", "unpadded"])
def test_strided_input(kc, extra_cols, pad):
    net, lengths, utts = case_input("S", (1, 7, 23, 2), pad, 1520)
    check_levels("S", net, 8, utts, lengths, pad, padded(np.concatenate(utts), extra_cols),
                 f"net S stride {8 + extra_cols}")


def test_state_after_a_shared_call(kc):
    kc.set_randn_seed(1530)
    net = kc.Nnet(SHARED_CONFIGS["S"])
    lengths = (7, 3)
    utts = utterances(lengths, 8, 1531)
    x = dev(np.concatenate(utts))
    y = net.Compute(x, list(lengths), apply_log=True, share_time=True)
    assert y.shape == (10, 10)
    dy = dev(np.zeros((10, 10), F32))
    labels = [(i, i % 10, 1.0) for i in range(10)]
    for call in (lambda: net.BackpropXent(labels), lambda: net.Backprop(dy),
                 lambda: net.BackpropComponent(net.NumComponents() - 1, dy)):
        with pytest.raises(kc.KcnnError, match="propagate first"):
            call()
    # the activations below the gathered one were never formed
    for i in range(7):
        with pytest.raises(kc.KcnnError, match="time maps"):
            net.Output(i)
    assert net.Output(7).shape == (10, 128) and net.Output(-1).shape == (10, 8)
    # the last output is there on request, the Softmax not having run
    p = host(net.Output()).copy()
    assert_same(p, host(net.Compute(x, list(lengths), share_time=True)), "P after the shared call")
    # after a Propagate the network trains again, and TimeMap is gone
    net.Propagate(dev(windows(utts, 5, 5)))
    net.BackpropXent(labels)
    assert net.ObjfTotal()[1] == 10
    with pytest.raises(kc.KcnnError, match="kcnn_nnet_compute_shared"):
        net.TimeMap(1)


def test_repeated_and_interleaved_calls(kc):
    """Batches of other sizes in turn, and each pass after the other: every
    call gives the bits its own first call gave."""
    net = shared_net("S")
    batches = [(1, 37, 5, 300), (11,), (64, 2), (1,), (1, 37, 5, 300)]
    first = {}
    for share in (True, False, True, True, False):
        for i, lengths in enumerate(batches):
            utts = utterances(lengths, 8, 1540 + len(lengths))
            y = host(net.Compute(dev(np.concatenate(utts)), list(lengths), apply_log=True,
                                 share_time=share)).copy()
            key = (share, lengths)
            if key in first:
                assert_same(y, first[key], f"{'shared' if share else 'own'} {lengths} again")
            first[key] = y


def test_refused_lengths_run_nothing(kc):
    net = shared_net("S")
    (x,) = utterances((9,), 8, 1550)
    view = net.Compute(dev(x), share_time=True)
    before = host(view).copy()
    for lengths in ([4, 4], [0, 9], [-1, 10], [], [9, 1]):
        with pytest.raises(kc.KcnnError, match="kcnn_nnet_compute_shared"):
            net.Compute(dev(x), lengths, share_time=True)
    with pytest.raises(kc.KcnnError, match="at least 11"):
        net.Compute(dev(x), pad_input=False, share_time=True)  # T <= L + R
    assert_same(host(view), before, "the last result after the refused calls")
    assert net.TimeMap(1)[1:] == (32, 8, 1)


# ---- 6. nnet.config's test model --------------------------------------------------------
def test_nnet_config_two_short_utterances(kc):
    net = nnet_config_model()
    lengths = (3, 8)
    utts = utterances(lengths, 40, 1600)
    x = dev(np.concatenate(utts))
    y, y_own = check_levels("nnet", net, 14, utts, lengths, True, x, "nnet.config")
    assert_same(host(net.Compute(x, list(lengths), share_time=True)), y, "the shared pass again")
    chain = [net.TimeMap(lvl)[1:] for lvl in (0, 1, 7, 8, 13)]
    assert chain == [(1, 21, 1), (128, 18, 1), (256, 12, 1), (256, 6, 2), (512, 2, 2)]
    assert np.isfinite(y).all() and y.shape == y_own.shape == (11, 3454)
