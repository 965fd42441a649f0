"""Compute(share_time=True) and OnlineComputer(share_time=True) on networks that
convolve along frequency: time maps whose levels keep a height, (C, H, n,
delta), a map row holding H C floats with element (h, c) at column h + c H
(capi/time-plan.h).  The six checks of tests/test_gpu_compute_shared.py on

  F  c2 shrunken: Splice d 7, L 2, R 3 (n 6); conv 3 x 1 -> 6 (H 5); pool 1 x 1
     x 3; ReLU 60; FC 60 -> 9; Softmax.  Prefix 4.
  M  every kind of level: Splice d 8, L 3, R 3 (n 7); conv 3 x 2 -> 8 (H 6, n
     6); ReLU; pool 2 x 2 x 1 (H 3, n 3, delta 2); ReLU; conv 2 x 2 -> 12 (H 2,
     n 2); ReLU; conv 2 x 2 -> 16 over the full height (H 1, n 1); ReLU; FC 16
     -> 10; Softmax.  Prefix 9.

1. Levels: TimeMap(l) / TimeMapHeight(l) at its valid rows against TimeMap(l -
   1).  A convolution against fp64 under assert_bound(rtol=1e-5) with S = sum
   |terms| + |b|; pool and ReLU bit-exact against a numpy fp32 restatement of
   the reference's fold (c outer, w, h inner); level 0 bit-exact against the
   (clamped) frames; Output(prefix - 1) bit-exact against numpy indexing of the
   last map.
2. Against Compute: Output(prefix - 1) of the two passes differs by at most 2
   E, E the per-layer bar propagated in fp64 (E' = |W| (*) E + 1e-5 S through a
   convolution, the window maximum of E through a pool, unchanged through a
   ReLU): derived from the bar, not measured.
3. Integer data (inputs in {-2..2}, weights in {-1, 0, 1} with at most 4
   non-zeros a filter, integer biases, every activation below 2^11, asserted on
   the reference): Output(prefix - 1) of both passes equals the oracle's window
   pass (O.Conv, O.Pool) bit for bit and the results are bit-identical.
4. Utterances of (1, 7, 23, 2) frames padded, and that many RESULT frames
   unpadded (checks 1 to 3 run on them).
5. The literal path: prefix 0, Compute's bits.
6. Streaming: OnlineComputer(M, 3, 4, share_time=True) beside the default
   computer through a schedule with a final, a Reset and a reused slot; Output(
   prefix - 1) within 2 E and the results within the bound
   tests/test_gpu_online_shared.py derives from E; on integer data to the bit.
Also the prefixes kcnn_nnet_time_shared_prefix gives for F, M and
tests/golden/freq_conv.config (4, 9, 4), and freq_conv.config's levels."""
import functools
import os

import numpy as np
import pytest

import oracle as O
from _util import assert_bound, assert_same, dev, host, rng
from test_gpu_compute import FC, utterances, windows
from test_gpu_compute_shared import Geometry, line_args
from test_gpu_online import Model, results_equal, run_steps
from test_gpu_online_shared import upper_scale

pytestmark = pytest.mark.gpu

F32 = np.float32
RTOL = 1e-5
OPTS = ("learning-rate=0.02 param-stddev=0.3 bias-stddev=0.5 weight-decay=0.0005 momentum=0.9")


def conv(h, w, c, kh, kw, g):
    return (f"ConvolutionComponent in-height={h} in-width={w} in-channel={c} kernel-height={kh} "
            f"kernel-width={kw} stride=1 group={g} out-height={h - kh + 1} out-width={w - kw + 1} "
            + OPTS)


def pool(h, w, c, ph, pw, pc):
    return (f"MaxpoolComponent in-height={h} in-width={w} in-channel={c} pool-height-dim={ph} "
            f"pool-width-dim={pw} pool-channel-dim={pc}")


NET_F = "\n".join([
    "SpliceComponent input-dim=7 left-context=2 right-context=3 const-component-dim=0",
    conv(7, 6, 1, 3, 1, 6), pool(5, 6, 6, 1, 1, 3), "RectifiedLinearComponent dim=60",
    FC.format(i=60, o=9, s=0.3), "SoftmaxComponent dim=9"])
NET_M = "\n".join([
    "SpliceComponent input-dim=8 left-context=3 right-context=3 const-component-dim=0",
    conv(8, 7, 1, 3, 2, 8), "RectifiedLinearComponent dim=288", pool(6, 6, 8, 2, 2, 1),
    "RectifiedLinearComponent dim=72", conv(3, 3, 8, 2, 2, 12), "RectifiedLinearComponent dim=48",
    conv(2, 2, 12, 2, 2, 16), "RectifiedLinearComponent dim=16", FC.format(i=16, o=10, s=0.3),
    "SoftmaxComponent dim=10"])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freq_conv.config")
CONFIGS = {"F": NET_F, "M": NET_M}
PREFIX = {"F": 4, "M": 9}
# (C, H, n, delta) of every level
CHAIN = {"F": [(1, 7, 6, 1), (6, 5, 6, 1), (2, 5, 6, 1), (2, 5, 6, 1)],
         "M": [(1, 8, 7, 1), (8, 6, 6, 1), (8, 6, 6, 1), (8, 3, 3, 2), (8, 3, 3, 2), (12, 2, 2, 2),
               (12, 2, 2, 2), (16, 1, 1, 2), (16, 1, 1, 2)]}
FRAMES = (1, 7, 23, 2)


def args_of(name):
    return [line_args(ln) for ln in CONFIGS[name].splitlines()]


@functools.lru_cache(maxsize=None)
def height_net(name):
    import kcnn
    kcnn.init(0)
    kcnn.set_randn_seed(6100 + ord(name))
    return kcnn.Nnet(CONFIGS[name])


# ---- one level in numpy -----------------------------------------------------------------
def unfold(a, rows, H, C, kh, kw, delta):
    """A[(r, oh), i + d kh + c kh kw] = a[rows[r] + delta d, oh + i + c H]."""
    OH = H - kh + 1
    out = np.empty((len(rows), OH, kh * kw * C), a.dtype)
    for c in range(C):
        for d in range(kw):
            for i in range(kh):
                out[:, :, i + d * kh + c * kh * kw] = a[rows + delta * d][:, i + c * H:i + c * H + OH]
    return out.reshape(len(rows) * OH, -1)


def to_map(t, nrows, OH, G):
    """[(r, oh), g] -> [r, oh + g OH]."""
    return np.ascontiguousarray(t.reshape(nrows, OH, G).transpose(0, 2, 1)).reshape(nrows, G * OH)


def fold(a, rows, H, ph, pw, pc, delta, start=F32(-1e20)):
    """The reference's Maxpool fold (start -1e20f, replace when v < x) over c <
    pc (outer), w < pw, h < ph (inner) of a[rows + delta w][oh ph + h + (oc pc
    + c) H], to [len(rows), oh + oc H']."""
    C = a.shape[1] // H
    OH, OC = H // ph, C // pc
    v = np.full((len(rows), OC, OH), start, a.dtype)
    for c in range(pc):
        for w in range(pw):
            x3 = a[rows + delta * w].reshape(len(rows), C, H)
            for h in range(ph):
                cand = x3[:, c::pc, h::ph]
                v = np.where(v < cand, cand, v)
    return v.reshape(len(rows), OC * OH)


def gather(geo, m, H, n, delta):
    """out[row(u, t)][h + k H + c H n] = m[base_u + t + delta k][h + c H]"""
    C = m.shape[1] // H
    out = np.empty((geo.total, C, n, H), m.dtype)
    for b, s, f in zip(geo.base, geo.start, geo.frames):
        for k in range(n):
            out[s:s + f, :, k, :] = m[b + delta * k:b + delta * k + f].reshape(f, C, H)
    return out.reshape(geo.total, C * n * H)


def read_maps(net):
    maps = []
    for lvl in range(net.TimeSharedPrefix()):
        view, c, n, d = net.TimeMap(lvl)
        maps.append((host(view).copy(), c, net.TimeMapHeight(lvl), n, d))
    return maps


def check_levels(name, net, utts, lengths, pad, what):
    """Checks 1 and 2 for one pass; returns (shared result, Compute's)."""
    args, prefix = args_of(name), PREFIX[name]
    geo = Geometry(net, lengths, pad)
    x = dev(np.concatenate(utts))
    assert net.TimeSharedPrefix() == prefix
    y = host(net.Compute(x, list(lengths), pad_input=pad, share_time=True)).copy()
    maps = read_maps(net)
    top = host(net.Output(prefix - 1)).copy()
    assert [m[1:] for m in maps] == CHAIN[name] and y.shape[0] == geo.total
    m0 = maps[0][0]
    assert m0.shape == (geo.input_rows, net.components[0].InputDim())
    assert_same(m0, geo.level0(utts), f"{what}: level 0")
    err = np.zeros(m0.shape)  # the bar E of each level, at every row (used at valid rows)
    kinds = [c.Type() for c in net.components]
    for lvl in range(1, prefix):
        a, C_in, H_in, n_in, d_in = maps[lvl - 1]
        got, C, H, n, d = maps[lvl]
        assert got.shape[1] == C * H
        rows = geo.valid(n, d)
        assert rows.max() < got.shape[0], (lvl, rows.max(), got.shape)
        e_out = np.zeros(got.shape)
        if kinds[lvl] == "ConvolutionComponent":
            kh, kw = args[lvl]["kernel-height"], args[lvl]["kernel-width"]
            comp = net.components[lvl]
            w64 = host(comp.LinearParams()).astype(np.float64)
            b64 = host(comp.BiasParams()).astype(np.float64)
            assert w64.shape == (kh * kw * C_in, C) and H == H_in - kh + 1
            au = unfold(a.astype(np.float64), rows, H_in, C_in, kh, kw, d_in)
            t = to_map(au @ w64 + b64, len(rows), H, C)
            s = to_map(np.abs(au) @ np.abs(w64) + np.abs(b64), len(rows), H, C)
            e = to_map(unfold(err, rows, H_in, C_in, kh, kw, d_in) @ np.abs(w64), len(rows), H, C)
            print(f"{what}: level {lvl} conv {kh} x {kw} x {C_in} -> {C}, height {H}: worst err / "
                  f"S = {(np.abs(got[rows] - t) / np.maximum(s, 1e-30)).max():.3e}")
            assert_bound(got[rows], t, s, rtol=RTOL, what=f"{what}: level {lvl} convolution")
            e_out[rows] = e + RTOL * s
        elif kinds[lvl] == "MaxpoolComponent":
            ph, pw, pc = (args[lvl][k] for k in ("pool-height-dim", "pool-width-dim",
                                                 "pool-channel-dim"))
            assert_same(got[rows], fold(a, rows, H_in, ph, pw, pc, d_in), f"{what}: level {lvl} pool")
            e_out[rows] = fold(err, rows, H_in, ph, pw, pc, d_in, start=0.0)
        else:
            assert kinds[lvl] == "RectifiedLinearComponent"
            assert_same(got[rows], np.where(a[rows] < 0, F32(0), a[rows]),
                        f"{what}: level {lvl} ReLU")
            e_out[rows] = err[rows]
        err = e_out
    last, C, H, n, d = maps[-1]
    assert top.shape == (geo.total, C * H * n)
    assert_same(top, gather(geo, last, H, n, d), f"{what}: Output({prefix - 1}) is the gathered map")
    # check 2: Compute's own Output(prefix - 1), each within E of the truth
    y_own = host(net.Compute(x, list(lengths), pad_input=pad)).copy()
    top_own = host(net.Output(prefix - 1)).copy()
    bar = 2.0 * gather(geo, err, H, n, d)
    diff = np.abs(top.astype(np.float64) - top_own)
    print(f"{what}: worst |shared - Compute| / 2E = {(diff / np.maximum(bar, 1e-300)).max():.3e}")
    assert (diff <= bar).all(), \
        f"{what}: {(diff > bar).sum()} elements of Output differ by more than 2 E"
    assert y.shape == y_own.shape and np.isfinite(y).all()
    return y, y_own


def case_input(name, pad, seed, frames=FRAMES):
    net = height_net(name)
    context = net.LeftContext() + net.RightContext()
    lengths = tuple(frames) if pad else tuple(f + context for f in frames)
    return net, lengths, utterances(lengths, net.components[0].InputDim(), seed)


def test_prefixes(kc):
    kc.set_randn_seed(6000)
    golden = kc.Nnet(open(GOLDEN).read())
    assert [height_net("F").TimeSharedPrefix(), height_net("M").TimeSharedPrefix(),
            golden.TimeSharedPrefix()] == [4, 9, 4]
    # freq_conv.config's levels, on two short utterances
    x = dev(np.concatenate(utterances((3, 8), 40, 6001)))
    y = host(golden.Compute(x, [3, 8], share_time=True)).copy()
    chain = [golden.TimeMap(lvl)[1:] + (golden.TimeMapHeight(lvl),) for lvl in range(4)]
    assert chain == [(1, 11, 1, 40), (128, 11, 1, 33), (32, 11, 1, 33), (32, 11, 1, 33)]
    assert golden.TimeMap(1)[0].shape == (31, 33 * 128) and golden.Output(3).shape == (11, 11616)
    assert y.shape == (11, 3454) and np.isfinite(y).all()


@pytest.mark.parametrize("pad", [True, False], ids=["padded", "unpadded"])
@pytest.mark.parametrize("name", ["F", "M"])
def test_levels_and_against_compute(kc, name, pad):
    net, lengths, utts = case_input(name, pad, 6200 + ord(name))
    check_levels(name, net, utts, lengths, pad, f"net {name} {lengths}")


@pytest.mark.parametrize("name", ["F", "M"])
def test_one_short_utterance(kc, name):
    net, lengths, utts = case_input(name, True, 6210, frames=(1,))
    check_levels(name, net, utts, lengths, True, f"net {name} {lengths}")


# ---- 3. exact arithmetic ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_net(name):
    """The net with integer parameters in its prefix: weights in {-1, 0, 1},
    at most 4 non-zeros a filter, biases in {-2 .. 2}."""
    import torch
    import kcnn
    kcnn.init(0)
    kcnn.set_randn_seed(6300 + ord(name))
    net = kcnn.Nnet(CONFIGS[name])
    r = rng(6310 + ord(name))
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


def oracle_prefix(name, net, win):
    """The window pass of components 1 .. prefix - 1 by the oracle, in fp32;
    also the largest |activation|."""
    x, biggest = win, float(np.abs(win).max())
    args = args_of(name)
    for i in range(1, PREFIX[name]):
        comp, a = net.components[i], args[i]
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


def integer_utterances(net, lengths, seed):
    r = rng(seed)
    d = net.components[0].InputDim()
    return [r.integers(-2, 3, size=(t, d)).astype(F32) for t in lengths]


@pytest.mark.parametrize("pad", [True, False], ids=["padded", "unpadded"])
@pytest.mark.parametrize("name", ["F", "M"])
def test_integer_data_is_exact_and_the_result_bit_identical(kc, name, pad):
    net = integer_net(name)
    prefix = PREFIX[name]
    left, right = net.LeftContext(), net.RightContext()
    lengths = FRAMES if pad else tuple(f + left + right for f in FRAMES)
    utts = integer_utterances(net, lengths, 6400 + ord(name))
    if pad:
        win = windows(utts, left, right)
    else:
        span = left + right
        win = np.concatenate([u[t:t + span + 1] for u in utts for t in range(len(u) - span)])
    want, biggest = oracle_prefix(name, net, np.ascontiguousarray(win.reshape(sum(FRAMES), -1)))
    assert biggest < 2 ** 11, biggest
    assert (want == np.round(want)).all()
    x = dev(np.concatenate(utts))
    priors = (rng(6500).random(net.components[-1].OutputDim()) + 0.01).astype(F32)
    for kw in ({}, {"apply_log": True, "priors": priors, "prior_scale": 0.5}):
        y = host(net.Compute(x, list(lengths), pad_input=pad, share_time=True, **kw)).copy()
        top = host(net.Output(prefix - 1)).copy()
        y_own = host(net.Compute(x, list(lengths), pad_input=pad, **kw)).copy()
        top_own = host(net.Output(prefix - 1)).copy()
        print(f"net {name}: shared differs from the integers in {(top != want).sum()} of "
              f"{want.size}, Compute in {(top_own != want).sum()}; largest |activation| {biggest}")
        assert_same(top, want, f"net {name}: shared Output({prefix - 1}) against the integers")
        assert_same(top_own, want, f"net {name}: Compute's Output({prefix - 1})")
        assert_same(y, y_own, f"net {name}: the result {sorted(kw)}")


# ---- 5. the literal path -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["F", "M"])
def test_literal_path_gives_computes_bits(kc, name):
    net, lengths, utts = case_input(name, True, 6600)
    x = dev(np.concatenate(utts))
    try:
        kc.set_literal_path(True)
        assert net.TimeSharedPrefix() == 0
        own = host(net.Compute(x, list(lengths))).copy()
        assert_same(host(net.Compute(x, list(lengths), share_time=True)), own, "literal")
        with pytest.raises(kc.KcnnError, match="kcnn_nnet_compute_shared"):
            net.TimeMapHeight(0)
    finally:
        kc.set_literal_path(False)
    assert net.TimeSharedPrefix() == PREFIX[name]


def test_repeated_calls_give_the_same_bits(kc):
    net, lengths, utts = case_input("M", True, 6610)
    x = dev(np.concatenate(utts))
    first = host(net.Compute(x, list(lengths), share_time=True)).copy()
    top = host(net.Output(8)).copy()
    net.Compute(x, list(lengths))
    assert_same(host(net.Compute(x, list(lengths), share_time=True)), first, "the shared pass again")
    assert_same(host(net.Output(8)), top, "Output(8) again")


# ---- 6. streaming ------------------------------------------------------------------------
STREAMS, MAX_CHUNK = 3, 4
STREAM_LENGTHS = (1, 9, 6, 3)   # L = R = 3: T = 1, 9, 6, 3 = R
# (slot, utterance, new frames, final): slot 0 ends utterance 0 (T = 1) in its first
# step and is reused for utterance 3; slot 2's first chunk is shorter than R + 1
SCHEDULE = (
    ((0, 0, 1, True), (1, 1, 4, False), (2, 2, 2, False)),
    ((0, 3, 3, True), (1, 1, 4, False)),
    ((2, 2, 1, False),),                       # no slot emits
    ((1, 1, 1, True), (2, 2, 3, True)),        # finals with frames
)
# after a Reset of slot 2 (utterance 1's first frames abandoned in it)
AFTER_RESET = (((2, 2, 4, False),), ((2, 2, 2, False), (0, 0, 1, True)), ((2, 2, 0, True),))


def truth_maps(name, net, x):
    """The gathered last time map of one whole utterance in fp64, [T x C n H],
    and the bar E at each of its elements (S on the fp64 maps, 0.1 % added, as
    tests/test_gpu_online_shared.py takes it)."""
    left, right = net.LeftContext(), net.RightContext()
    args, kinds = args_of(name), [c.Type() for c in net.components]
    t_len = len(x)
    cur = x[np.clip(np.arange(-left, t_len + right), 0, t_len - 1)].astype(np.float64)
    err = np.zeros_like(cur)
    C, H, n, delta = CHAIN[name][0]
    for lvl in range(1, PREFIX[name]):
        if kinds[lvl] == "ConvolutionComponent":
            kh, kw = args[lvl]["kernel-height"], args[lvl]["kernel-width"]
            comp = net.components[lvl]
            w64 = host(comp.LinearParams()).astype(np.float64)
            b64 = host(comp.BiasParams()).astype(np.float64)
            rows = np.arange(cur.shape[0] - delta * (kw - 1))
            OH, G = H - kh + 1, w64.shape[1]
            au = unfold(cur, rows, H, C, kh, kw, delta)
            s = to_map(np.abs(au) @ np.abs(w64) + np.abs(b64), len(rows), OH, G)
            e = to_map(unfold(err, rows, H, C, kh, kw, delta) @ np.abs(w64), len(rows), OH, G)
            cur, err = to_map(au @ w64 + b64, len(rows), OH, G), e + RTOL * s * 1.001
            C, H, n = G, OH, n - kw + 1
        elif kinds[lvl] == "MaxpoolComponent":
            ph, pw, pc = (args[lvl][k] for k in ("pool-height-dim", "pool-width-dim",
                                                 "pool-channel-dim"))
            rows = np.arange(cur.shape[0] - delta * (pw - 1))
            cur = fold(cur, rows, H, ph, pw, pc, delta, start=-1e20)
            err = fold(err, rows, H, ph, pw, pc, delta, start=0.0)
            C, H, n, delta = C // pc, H // ph, n // pw, delta * pw
        else:
            cur = np.maximum(cur, 0.0)
    assert (C, H, n, delta) == CHAIN[name][-1] and cur.shape[0] >= t_len + delta * (n - 1)

    def windows_of(m):
        out = np.empty((t_len, C, n, H))
        for k in range(n):
            out[:, :, k, :] = m[delta * k:delta * k + t_len].reshape(t_len, C, H)
        return out.reshape(t_len, -1)
    return windows_of(cur), windows_of(err)


def computers(kc, net):
    own = kc.OnlineComputer(net, STREAMS, MAX_CHUNK)
    shared = kc.OnlineComputer(net, STREAMS, MAX_CHUNK, share_time=True)
    assert shared.TimeSharedPrefix() == 9 and own.TimeSharedPrefix() == 0
    return own, shared


def abandon_and_reset(oc, utts, right):
    """Utterance 1's first frames into slot 2, then Reset."""
    other = Model(right, STREAM_LENGTHS)
    run_steps(oc, other, utts, (((2, 1, 4, False),), ((2, 1, 2, False),)), streams=0)
    assert oc.Frames(2) == (6, 3)
    oc.Reset(2)
    assert oc.Frames(2) == (0, 0)


def test_streaming_against_the_default_computer(kc):
    net = height_net("M")
    utts = utterances(STREAM_LENGTHS, 8, 6700)
    own, shared = computers(kc, net)
    right = net.RightContext()
    truth = [truth_maps("M", net, x) for x in utts]
    bound = [upper_scale(net, 9, t, e) for t, e in truth]
    own_model, shared_model = Model(right, STREAM_LENGTHS), Model(right, STREAM_LENGTHS)
    quiet = 0
    for part in (SCHEDULE, AFTER_RESET):
        if part is AFTER_RESET:
            abandon_and_reset(shared, utts, right)
            abandon_and_reset(own, utts, right)
        for entries in part:
            ((emitted, y),) = run_steps(shared, shared_model, utts, (entries,), streams=STREAMS)
            top = host(net.Output(8)).copy() if emitted else None
            ((emitted_own, y_own),) = run_steps(own, own_model, utts, (entries,), streams=STREAMS)
            assert emitted == emitted_own and y.shape == y_own.shape
            if not emitted:
                quiet += 1
                continue
            top_own = host(net.Output(8)).copy()
            bar = 2.0 * np.stack([truth[u][1][t] for u, t in emitted])
            diff = np.abs(top.astype(np.float64) - top_own)
            print(f"{entries}: worst |shared - own| / 2E = "
                  f"{(diff / np.maximum(bar, 1e-300)).max():.3e}")
            assert top.shape == bar.shape and (diff <= bar).all(), \
                f"{entries}: {(diff > bar).sum()} elements of Output(8) differ by more than 2 E"
            lim = np.stack([bound[u][t] for u, t in emitted])
            diff = np.abs(y.astype(np.float64) - y_own)
            assert np.isfinite(y).all() and (diff <= lim + 1e-30).all(), \
                f"{entries}: {(diff > lim).sum()} elements of the result outside the bound"
    assert quiet >= 1 and not shared_model.slots and not own_model.slots


def test_streaming_integer_data_is_bit_identical(kc):
    net = integer_net("M")
    left, right = net.LeftContext(), net.RightContext()
    utts = integer_utterances(net, STREAM_LENGTHS, 6710)
    win = windows(utts, left, right).reshape(sum(STREAM_LENGTHS), -1)
    want, biggest = oracle_prefix("M", net, np.ascontiguousarray(win))
    assert biggest < 2 ** 11 and (want == np.round(want)).all()
    first = np.concatenate([[0], np.cumsum(STREAM_LENGTHS)])
    own, shared = computers(kc, net)
    own_model, shared_model = Model(right, STREAM_LENGTHS), Model(right, STREAM_LENGTHS)
    for part in (SCHEDULE, AFTER_RESET):
        if part is AFTER_RESET:
            abandon_and_reset(shared, utts, right)
            abandon_and_reset(own, utts, right)
        for entries in part:
            ((emitted, y),) = run_steps(shared, shared_model, utts, (entries,), streams=STREAMS)
            top = host(net.Output(8)).copy() if emitted else None
            got_own = run_steps(own, own_model, utts, (entries,), streams=STREAMS)
            results_equal([(emitted, y)], got_own, f"the result of {entries}")
            if emitted:
                rows = [first[u] + t for u, t in emitted]
                assert_same(top, want[rows], f"Output(8) of {entries}")
                assert_same(host(net.Output(8)), want[rows], f"the default's Output(8) of {entries}")
