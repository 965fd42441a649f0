"""Nnet.PropagateFrames(share_time=True) and the backward over time maps, on
the GPU: a training step whose convolutional prefix runs once per time step of
each run of consecutive corpus rows.

1. Each backward launch on its own inputs, read back after one step (TimeMap,
   TimeMapDeriv, InputDeriv(prefix), TimeGradient).  The scatter and the pool /
   ReLU backward bit-exact against a numpy fp32 restatement that sums in the
   kernel's stated order (k, then w, ascending); a convolution's data gradient
   and its weight and bias gradients against fp64 under assert_bound(rtol=1e-5)
   with S the sum of the absolute terms (the bar of the forward's convolutions:
   the same GEMMs).  Rows that no window reads are exactly 0 in every
   derivative map.
2. The applied step: W', b' and prev' of each prefix Convolution are
   ApplyGradient(TimeGradient(i), N) on a copy, bit for bit.
3. Integer data on a stack that ends in an FC with integer weights, driven by
   Backprop with an integer out_deriv: every sum exact (asserted on an fp64
   reference), so TimeGradient is the default step's ComputeGradient bit for
   bit and a twin stepped by PropagateFrames + Backprop ends with the same bits
   in every parameter.
4. Fallbacks: a net with a height level, the literal path: the default step's
   bits, training prefix 0.
5. State: refused calls, ReLU statistics, steps of both kinds in turn, Output
   below the prefix, refused lists.
6. train_epoch(chunk=k) is the hand-written loop.
7. nnet.config: one step on 2 runs of 8 frames, check 1 on all levels.

The corpus has utterances of 7, 23 and 40 frames (the first shorter than L + R
= 10: its run clamps at both ends); FRAMES is the list scripts/
time_backward_check.cc walks on the host."""
import os

import numpy as np
import pytest

from _util import assert_bound, assert_same, dev, host, rng, with_ties
from test_gpu_compute import FC, nnet_config_model, snapshot, assert_unchanged, utterances
from test_gpu_compute_shared import (PREFIX, SHARED_CONFIGS, config_lines, line_args, taps)
from test_gpu_train_frames import assert_bits, assert_same_state

pytestmark = pytest.mark.gpu

F32 = np.float32
RTOL = 1e-5
LENGTHS = (7, 23, 40)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _run(a, n):
    return list(range(a, a + n))


# the whole first utterance (clamps at both ends; starts at a first row and ends
# at a last row); rows 7.. follow it across the utterance boundary: a split; a
# run of 1; 25..29 ends utterance 1 and 30.. starts utterance 2: a split; the
# same run twice; three descending rows: three runs; a run ending at the last row
FRAMES = np.asarray(_run(0, 7) + _run(7, 5) + [41] + _run(25, 5) + _run(30, 6) + _run(50, 8) +
                    _run(50, 8) + [20, 19, 18] + _run(62, 8), np.int32)
RUNS = [(0, 7), (7, 5), (41, 1), (25, 5), (30, 6), (50, 8), (50, 8), (20, 1), (19, 1), (18, 1),
        (62, 8)]


def runs_of(frames, lengths):
    """The runs, naively: an entry continues the run before it when its row
    follows in the same utterance."""
    ends = np.cumsum(lengths)
    utt = lambda r: int(np.searchsorted(ends, r, side="right"))
    out = []
    for i, f in enumerate(frames):
        f = int(f)
        if i and f == int(frames[i - 1]) + 1 and utt(f) == utt(f - 1):
            out[-1] = (out[-1][0], out[-1][1] + 1)
        else:
            out.append((f, 1))
    return out


class Segments:
    """The rows of a training pass: run j has its first map row base[j] and
    gives k[j] result rows from start[j]."""

    def __init__(self, runs, context):
        self.k = [n for _, n in runs]
        self.start = [int(s) for s in np.cumsum([0] + self.k[:-1])]
        self.base = [s + j * context for j, s in enumerate(self.start)]
        self.input_rows = sum(self.k) + len(runs) * context

    def valid(self, n, delta, rows):
        mask = np.zeros(rows, bool)
        for b, k in zip(self.base, self.k):
            mask[b:b + k + delta * (n - 1)] = True
        return mask


def fresh(kc, name, seed):
    kc.set_randn_seed(seed)
    return kc.Nnet(SHARED_CONFIGS[name])


def corpus_of(kc, x):
    return kc.Corpus(dev(x), list(LENGTHS))


def labels_of(n, cols):
    return [(i, (7 * i) % cols, 1.0) for i in range(n)]


def pool_backward(inp, pooled, g, delta, pw, pc):
    """din[r][ch] = sum over w ascending of g[r - delta w][ch / pc] where
    in[r][ch] == pooled[r - delta w][ch / pc], in fp32."""
    rows = g.shape[0]
    din = np.zeros((rows + delta * (pw - 1), inp.shape[1]), F32)
    gg, pp = np.repeat(g, pc, axis=1), np.repeat(pooled[:rows], pc, axis=1)
    for w in range(pw):
        sl = slice(delta * w, delta * w + rows)
        din[sl] = din[sl] + np.where(inp[sl] == pp, gg, F32(0))
    return din


def check_backward(net, name, frames, lengths, w_before, what):
    """Check 1 after one step of `net` (config_lines(name)) on `frames`;
    w_before[i] = (W, b) of prefix Convolution i before the step."""
    p = net.TimeSharedTrainPrefix()
    args = [line_args(ln) for ln in config_lines(name)]
    kinds = [c.Type() for c in net.components]
    context = net.LeftContext() + net.RightContext()
    seg = Segments(runs_of(frames, lengths), context)
    maps = []
    for lvl in range(p):
        view, c, n, d = net.TimeMap(lvl)
        maps.append((host(view).copy(), c, n, d))
    assert maps[0][0].shape[0] == seg.input_rows
    dy = host(net.InputDeriv(p)).copy()
    assert dy.shape[0] == len(frames)

    def deriv(lvl):
        view, c, n, d = net.TimeMapDeriv(lvl)
        got = host(view).copy()
        assert (c, n, d) == maps[lvl][1:] and got.shape == (maps[lvl][0].shape[0], c)
        unread = ~seg.valid(n, d, got.shape[0])
        assert (got[unread] == 0).all(), f"{what}: level {lvl}: a row no window reads is not 0"
        return got

    # the scatter: dmap[base + t + delta k][c] += dy[start + t][k + c n], k ascending
    top, c, n, delta = maps[p - 1]
    want = np.zeros_like(top)
    for b, s, k in zip(seg.base, seg.start, seg.k):
        for pos in range(n):
            sl = slice(b + delta * pos, b + delta * pos + k)
            want[sl] = want[sl] + dy[s:s + k, pos::n]
    d_out = deriv(p - 1)
    assert_same(d_out, want, f"{what}: the scatter")
    with pytest.raises(Exception, match="no derivative map"):
        net.TimeMapDeriv(0)
    lvl = p - 1
    while lvl >= 1:
        rows = d_out.shape[0]
        below = lvl - 1
        if kinds[lvl] == "RectifiedLinearComponent" and kinds[lvl - 1] == "MaxpoolComponent":
            pw, pc = args[lvl - 1]["pool-width-dim"], args[lvl - 1]["pool-channel-dim"]
            below = lvl - 2
            inp, d_in = maps[below][0], maps[below][3]
            g = np.where(maps[lvl][0] > 0, d_out, F32(0))
            pp = np.repeat(maps[lvl - 1][0], pc, axis=1)
            routed = sum(int((inp[d_in * w:d_in * w + rows] == pp).sum()) for w in range(pw))
            print(f"{what}: level {lvl - 1} pool: {routed - maps[lvl - 1][0].size} tied maxima")
            want = pool_backward(inp, maps[lvl - 1][0], g, d_in, pw, pc)
            with pytest.raises(Exception, match="no derivative map"):
                net.TimeMapDeriv(lvl - 1)
            got = deriv(below)
            assert_same(got, want, f"{what}: level {lvl - 1} pool + ReLU backward")
        elif kinds[lvl] == "RectifiedLinearComponent":
            got = deriv(below)
            assert_same(got, np.where(maps[lvl][0] > 0, d_out, F32(0)),
                        f"{what}: level {lvl} ReLU backward")
        elif kinds[lvl] == "MaxpoolComponent":
            pw, pc = args[lvl]["pool-width-dim"], args[lvl]["pool-channel-dim"]
            got = deriv(below)
            assert_same(got, pool_backward(maps[below][0], maps[lvl][0], d_out, maps[below][3],
                                           pw, pc), f"{what}: level {lvl} pool backward")
        else:
            assert kinds[lvl] == "ConvolutionComponent"
            x, _, _, d_in = maps[below]
            w, b = w_before[lvl]
            kw = w.shape[0] // x.shape[1]
            on_splice = kinds[below] == "SpliceComponent"
            block = (lambda d: slice(d * x.shape[1], (d + 1) * x.shape[1])) if on_splice else \
                (lambda d: slice(d, None, kw))
            flat = host(net.TimeGradient(lvl)).copy()
            k_dim, g_dim = w.shape
            assert flat.shape == (k_dim * g_dim + g_dim,)
            gw, gb = flat[:k_dim * g_dim].reshape(k_dim, g_dim), flat[k_dim * g_dim:]
            x64, do64 = x.astype(np.float64), d_out.astype(np.float64)
            assert x.shape[0] == rows + d_in * (kw - 1)
            for d in range(kw):
                xd = x64[d_in * d:d_in * d + rows]
                assert_bound(gw[block(d)], xd.T @ do64, np.abs(xd).T @ np.abs(do64), rtol=RTOL,
                             what=f"{what}: level {lvl} weight gradient, tap {d}")
            assert_bound(gb, do64.sum(0), np.abs(do64).sum(0), rtol=RTOL,
                         what=f"{what}: level {lvl} bias gradient")
            if below >= 1:
                t, s = np.zeros(x.shape), np.zeros(x.shape)
                for d in range(kw):
                    sl = slice(d_in * d, d_in * d + rows)
                    w64 = w[block(d)].astype(np.float64)
                    t[sl] += do64 @ w64.T
                    s[sl] += np.abs(do64) @ np.abs(w64).T
                got = deriv(below)
                worst = (np.abs(got - t) / np.maximum(s, 1e-30)).max()
                print(f"{what}: level {lvl} data gradient: worst err / S = {worst:.3e}")
                assert_bound(got, t, s, rtol=RTOL, what=f"{what}: level {lvl} data gradient")
        lvl = below
        if lvl >= 1:
            d_out = got
    return maps


def prefix_convs(net):
    return [i for i in range(net.TimeSharedPrefix())
            if net.components[i].Type() == "ConvolutionComponent"]


def params_before(net):
    return {i: (host(net.components[i].LinearParams()).copy(),
                host(net.components[i].BiasParams()).copy()) for i in prefix_convs(net)}


def tied_weights(net, seed):
    """Prefix weights and biases quantised to quarters, so that products and
    sums are exact and pool windows hold ties."""
    import torch
    r = rng(seed)
    for i in prefix_convs(net):
        comp = net.components[i]
        k, g = comp.ParamDim(0)
        comp.SetParam(0, torch.from_numpy(with_ties(r, (k, g), levels=2)).cuda())
        comp.SetParam(1, torch.from_numpy(with_ties(r, (g,), levels=2)).cuda())


# ---- 1, 2: every launch, and the applied step ---------------------------------------------
@pytest.mark.parametrize("name", ["S", "P"])
@pytest.mark.parametrize("ties", [False, True], ids=["gaussian", "ties"])
def test_each_backward_launch_and_the_applied_step(kc, name, ties):
    net = fresh(kc, name, 6100 + ord(name))
    assert net.TimeSharedTrainPrefix() == PREFIX[name] == 8
    if ties:
        tied_weights(net, 6150)
        x = with_ties(rng(6101), (sum(LENGTHS), 8))
    else:
        x = np.concatenate(utterances(LENGTHS, 8, 6102))
    assert runs_of(FRAMES, LENGTHS) == RUNS
    corpus = corpus_of(kc, x)
    twin = net.Copy()
    before = params_before(net)
    n = len(FRAMES)
    net.PropagateFrames(corpus, FRAMES, share_time=True)
    # level 0: every example's clamped context
    m0 = host(net.TimeMap(0)[0])
    seg = Segments(RUNS, 10)
    ends = np.cumsum(LENGTHS)
    at = 0
    for (r0, k), b in zip(RUNS, seg.base):
        u = int(np.searchsorted(ends, r0, side="right"))
        lo, hi = int(ends[u] - LENGTHS[u]), int(ends[u] - 1)
        assert_same(m0[b:b + k + 10], x[np.clip(np.arange(r0 - 5, r0 + k + 5), lo, hi)], "level 0")
        at += k
    assert at == n and net.Output().shape == (n, 10)
    net.BackpropXent(labels_of(n, 10))
    check_backward(net, name, FRAMES, LENGTHS, before, f"net {name}")
    # 2. the applied step
    for i in prefix_convs(net):
        twin.components[i].ApplyGradient(net.TimeGradient(i), n)
        for which, label in ((0, "W"), (1, "b"), (2, "prev")):
            assert_bits(host(net.components[i].GetParam(which)),
                        host(twin.components[i].GetParam(which)), f"net {name} conv {i} {label}'")
        assert not np.array_equal(host(net.components[i].LinearParams()), before[i][0])


# ---- 3. exact arithmetic ------------------------------------------------------------------
def integer_stack(kc, name):
    """The prefix of net `name` and an FC, every parameter an integer: weights
    in {-1, 0, 1} with at most 4 (the FC: 3) non-zeros a filter, biases in {-2 ..
    2}."""
    import torch
    lines = config_lines(name)[:PREFIX[name]]
    top = line_args(lines[-1])["dim"]
    kc.set_randn_seed(6200 + ord(name))
    net = kc.Nnet("\n".join(lines + [FC.format(i=top, o=6, s=0.3)]))
    r = rng(6300 + ord(name))
    for comp, most in [(net.components[i], 4) for i in prefix_convs(net)] + [(net.components[-1], 3)]:
        k, g = comp.ParamDim(0)
        w = np.zeros((k, g), F32)
        if comp.Type() == "ConvolutionComponent":
            for col in range(g):
                at = r.choice(k, size=min(most, k), replace=False)
                w[at, col] = r.choice([-1.0, 1.0], size=len(at))
            bias = g
        else:  # [output x input]
            for row in range(k):
                at = r.choice(g, size=most, replace=False)
                w[row, at] = r.choice([-1.0, 1.0], size=most)
            bias = k
        comp.SetParam(0, torch.from_numpy(w).cuda())
        comp.SetParam(1, torch.from_numpy(r.integers(-2, 3, size=bias).astype(F32)).cuda())
    return net


@pytest.mark.parametrize("name", ["S", "P"])
def test_integer_data_is_exact_and_the_step_bit_identical(kc, name):
    net = integer_stack(kc, name)
    assert net.TimeSharedTrainPrefix() == 8 and net.NumComponents() == 9
    twin, ref = net.Copy(), net.Copy()
    x = rng(6400 + ord(name)).integers(-2, 3, size=(sum(LENGTHS), 8)).astype(F32)
    corpus = corpus_of(kc, x)
    n = len(FRAMES)
    r = rng(6500)
    dy = np.where(r.random((n, 6)) < 0.25, r.choice([-1.0, 1.0], size=(n, 6)), 0.0).astype(F32)
    before = params_before(net)
    net.PropagateFrames(corpus, FRAMES, share_time=True)
    net.Backprop(dev(dy))
    twin.PropagateFrames(corpus, FRAMES)
    top, top_own = host(net.Output(7)).copy(), host(twin.Output(7)).copy()
    assert_same(top, top_own, f"net {name}: Output(7)")
    twin.Backprop(dev(dy))
    # every sum is exact: on the fp64 reference every map, derivative and sum of
    # absolute terms is an integer below 2^11 (operands: one f16 part) / 2^24
    maps = check_backward(net, name, FRAMES, LENGTHS, before, f"integer net {name}")
    biggest = max(float(np.abs(m[0]).max()) for m in maps)
    assert biggest < 2 ** 11, biggest
    for lvl in range(1, 8):
        try:
            d = host(net.TimeMapDeriv(lvl)[0]).astype(np.float64)
        except kc.KcnnError:
            continue
        assert (d == np.round(d)).all() and np.abs(d).max() < 2 ** 11, (lvl, np.abs(d).max())
        if net.components[lvl].Type() == "ConvolutionComponent":
            m = maps[lvl - 1][0].astype(np.float64)
            rows = d.shape[0]
            s = max(float((np.abs(m[o:o + rows]).T @ np.abs(d)).max())
                    for o in range(m.shape[0] - rows + 1))
            assert s < 2 ** 24, (lvl, s)
    # TimeGradient is the default step's ComputeGradient
    for i in prefix_convs(net):
        want = ref.components[i].ComputeGradient(twin.Output(i - 1), twin.InputDeriv(i + 1))
        got = host(net.TimeGradient(i))
        assert (got == np.round(got)).all()
        assert_bits(got, host(want), f"integer net {name}: TimeGradient({i})")
    # (the parameters alone: the prefix ReLUs of `net` accumulated no statistics)
    mine, theirs = snapshot(net)[0], snapshot(twin)[0]
    assert len(mine) == len(theirs) == 3 * 4
    for k, (a, b) in enumerate(zip(mine, theirs)):
        assert_bits(host(a), host(b), f"integer net {name}: parameter block {k} after the step")


# ---- 4. fallbacks --------------------------------------------------------------------------
def default_and_shared_step(kc, base, corpus, frames, labels):
    a, b = base.Copy(), base.Copy()
    a.PropagateFrames(corpus, frames)
    out_a = host(a.Output()).copy()
    a.BackpropXent(labels)
    b.PropagateFrames(corpus, frames, share_time=True)
    out_b = host(b.Output()).copy()
    b.BackpropXent(labels)
    return a, b, out_a, out_b


def test_a_net_with_a_height_level_takes_the_default_step(kc):
    kc.set_randn_seed(6600)
    base = kc.Nnet(open(os.path.join(GOLDEN, "freq_conv.config")).read())
    assert base.TimeSharedPrefix() > 0 and base.TimeSharedTrainPrefix() == 0
    d = base.components[0].InputDim()
    x = np.concatenate(utterances(LENGTHS, d, 6601))
    labels = labels_of(len(FRAMES), base.components[-1].OutputDim())
    a, b, out_a, out_b = default_and_shared_step(kc, base, corpus_of(kc, x), FRAMES, labels)
    assert_bits(out_a, out_b, "freq_conv.config: the output")
    assert_same_state(kc, a, b, "freq_conv.config: the step")
    with pytest.raises(kc.KcnnError, match="kcnn_nnet_time_map_deriv"):
        b.TimeMapDeriv(1)


def test_the_literal_path_takes_the_default_step(kc):
    base = fresh(kc, "S", 6700)
    x = np.concatenate(utterances(LENGTHS, 8, 6701))
    try:
        kc.set_literal_path(True)
        assert base.TimeSharedTrainPrefix() == 0
        a, b, out_a, out_b = default_and_shared_step(kc, base, corpus_of(kc, x), FRAMES[:20],
                                                     labels_of(20, 10))
    finally:
        kc.set_literal_path(False)
    assert base.TimeSharedTrainPrefix() == 8
    assert_bits(out_a, out_b, "literal path: the output")
    assert_same_state(kc, a, b, "literal path: the step")


# ---- 5. state ------------------------------------------------------------------------------
def test_refused_calls_change_nothing_and_relu_statistics_stay(kc):
    net = fresh(kc, "S", 6800)
    x = np.concatenate(utterances(LENGTHS, 8, 6801))
    corpus = corpus_of(kc, x)
    n = len(FRAMES)
    labels = labels_of(n, 10)
    net.PropagateFrames(corpus, FRAMES)  # a default step first: the statistics are not zero
    net.BackpropXent(labels)
    relus = [i for i in range(8) if net.components[i].Type() == "RectifiedLinearComponent"]
    stats = [net.components[i].NonlinearStats() for i in relus]
    assert all(s[2] > 0 for s in stats)
    net.PropagateFrames(corpus, FRAMES, share_time=True)
    before = snapshot(net)
    out = host(net.Output()).copy()
    dy = dev(np.zeros((n, 256), F32))
    import torch
    grad = torch.zeros(net.components[3].NumGradientParams(), device="cuda")
    for i in range(7):
        with pytest.raises(kc.KcnnError, match="time maps"):
            net.Output(i)
    assert net.Output(7).shape == (n, 128) and net.TimeMap(7)[1:] == (64, 2, 2)
    for who, call in (("kcnn_nnet_backprop_component", lambda: net.BackpropComponent(3, dy)),
                      ("kcnn_nnet_backprop_component", lambda: net.BackpropComponent(0, dy)),
                      ("kcnn_nnet_backprop_component",
                       lambda: net.BackpropComponent(3, dy, mode=1, grad=grad)),
                      ("kcnn_nnet_backprop_component",
                       lambda: net.BackpropComponent(6, dy, mode=3, grad=grad)),
                      ("kcnn_nnet_backprop_split",
                       lambda: net.BackpropSplit(3, dy, grad, False, None)),
                      ("kcnn_nnet_input_deriv", lambda: net.InputDeriv(3)),
                      ("kcnn_nnet_input_deriv", lambda: net.InputDeriv(7)),
                      ("kcnn_nnet_time_map_deriv", lambda: net.TimeMapDeriv(7)),
                      ("kcnn_nnet_time_gradient", lambda: net.TimeGradient(1))):
        with pytest.raises(kc.KcnnError, match=who):
            call()
    # refused lists run nothing: an index outside the corpus; 3.2 million runs of
    # one frame, whose widest map (35.2 million rows of 64) reaches 2^31 elements
    # while every activation of the default pass (256 columns) stays below
    for bad, why in (([0, 70], "outside"), ([-1], "outside"), ([], "no frames"),
                     (np.full(3_200_000, 3, np.int32), "2\\^31")):
        with pytest.raises(kc.KcnnError, match=why):
            net.PropagateFrames(corpus, bad, share_time=True)
    assert_unchanged(before, snapshot(net))
    assert_bits(host(net.Output()), out, "the output after the refused calls")
    net.BackpropXent(labels)  # the shared forward still stands
    assert net.TimeGradient(1).shape == (8 * 4 * 32 + 32,)
    with pytest.raises(kc.KcnnError, match="not a Convolution"):
        net.TimeGradient(2)
    with pytest.raises(kc.KcnnError, match="not a Convolution"):
        net.TimeGradient(8)
    for i, (vs, ds, cnt) in zip(relus, stats):
        vs1, ds1, cnt1 = net.components[i].NonlinearStats()
        np.testing.assert_array_equal(vs, vs1)
        np.testing.assert_array_equal(ds, ds1)
        assert cnt == cnt1
    assert net.ObjfTotal()[1] == 2 * n


def test_steps_of_both_kinds_in_turn(kc):
    """A default step right after a shared one, and the reverse, against a
    copy that never ran the other kind."""
    x = np.concatenate(utterances(LENGTHS, 8, 6901))
    corpus = corpus_of(kc, x)
    other = np.asarray(_run(33, 9) + _run(2, 4) + [69], np.int32)
    for first_shared in (True, False):
        net = fresh(kc, "P", 6900)
        net.PropagateFrames(corpus, FRAMES, share_time=first_shared)
        net.BackpropXent(labels_of(len(FRAMES), 10))
        only = net.Copy()  # the same parameters, none of the state
        net.ObjfTotal(reset=True)
        for m in (net, only):
            m.PropagateFrames(corpus, other, share_time=not first_shared)
        assert_bits(host(net.Output()), host(only.Output()), "the second forward")
        for m in (net, only):
            m.BackpropXent(labels_of(len(other), 10))
        assert_same_state(kc, net, only, f"the step after a {'shared' if first_shared else 'default'} one")
        if first_shared:
            assert host(net.InputDeriv(3)).shape[0] == len(other)
            with pytest.raises(kc.KcnnError, match="kcnn_nnet_time_map"):
                net.TimeMap(1)
        else:
            for i in prefix_convs(net):
                assert_bits(host(net.TimeGradient(i)), host(only.TimeGradient(i)), f"TimeGradient({i})")


# ---- 6. train_epoch(chunk=k) ---------------------------------------------------------------
def test_train_epoch_with_chunks_is_the_hand_written_loop(kc):
    base = fresh(kc, "S", 7000)
    x = np.concatenate(utterances(LENGTHS, 8, 7001))
    corpus = corpus_of(kc, x)
    pdfs = rng(7002).integers(0, 10, size=sum(LENGTHS)).astype(np.int32)
    chunk, mb = 8, 20  # 2 runs a minibatch
    runs = [(0, 7), (7, 8), (15, 8), (23, 7), (30, 8), (38, 8), (46, 8), (54, 8), (62, 8)]
    assert kc.chunk_runs(LENGTHS, chunk) == runs
    net = base.Copy()
    seen = []
    inner = net.PropagateFrames

    def recording(c, f, share_time=False):
        seen.append((np.array(f, np.int32), share_time))
        inner(c, f, share_time=share_time)
    net.PropagateFrames = recording
    got = kc.train_epoch(net, corpus, pdfs, mb, srand=3, chunk=chunk)
    order = np.random.default_rng(3).permutation(len(runs))
    twin = base.Copy()
    lists = []
    for at in range(0, len(runs), 2):
        fr = np.concatenate([np.arange(runs[j][0], runs[j][0] + runs[j][1], dtype=np.int32)
                             for j in order[at:at + 2]])
        lists.append(fr)
        twin.PropagateFrames(corpus, fr, share_time=True)
        twin.BackpropXent([(i, int(pdfs[r]), 1.0) for i, r in enumerate(fr)])
    assert len(seen) == 5 and all(s for _, s in seen)
    for (f, _), want in zip(seen, lists):
        np.testing.assert_array_equal(f, want)
    assert sorted(np.concatenate(lists).tolist()) == list(range(sum(LENGTHS)))
    want = twin.ObjfTotal(reset=True)
    assert got == want and got[1] == sum(LENGTHS), (got, want)
    assert_same_state(kc, net, twin, "train_epoch(chunk=8) against the loop")
    with pytest.raises(kc.KcnnError, match="chunk"):
        kc.train_epoch(net, corpus, pdfs, mb, chunk=0)


# ---- 7. nnet.config ------------------------------------------------------------------------
def test_nnet_config_two_runs_of_eight(kc):
    net = nnet_config_model().Copy()
    assert net.TimeSharedTrainPrefix() == 14
    lengths = (30, 12)
    x = np.concatenate(utterances(lengths, 40, 7100))
    corpus = kc.Corpus(dev(x), list(lengths))
    frames = np.asarray(_run(5, 8) + _run(32, 8), np.int32)
    before = params_before(net)
    net.PropagateFrames(corpus, frames, share_time=True)
    net.BackpropXent(labels_of(16, net.components[-1].OutputDim()))
    check_backward(net, "nnet", frames, lengths, before, "nnet.config")
    assert [net.TimeMapDeriv(lvl)[1:] for lvl in (1, 7, 9, 13)] == \
        [(128, 18, 1), (256, 12, 1), (256, 6, 2), (512, 2, 2)]
