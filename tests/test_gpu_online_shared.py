"""OnlineComputer(share_time=True): a step's leading Splice -> {Convolution |
Maxpool | ReLU}... components once per time step of the frames its slots hold
(time maps) instead of once per emitted frame's window, on the GPU.

One computer of each kind on the same net is fed the SCHEDULE of
tests/test_gpu_online.py (T = 1, a first chunk shorter than R + 1, final alone,
one frame a step, slot reuse, a step that emits nothing) on the nets of
tests/test_gpu_compute_shared.py: A, B, the shrunken nnet.config (S) and its
channel-pool variant (P).  After each step
  * the counts and Frames are the model's, for both;
  * Output(prefix - 1) of the two differ by at most 2 E.  E is the bar of
    check 2 of test_gpu_compute_shared.py, propagated in fp64 over the time
    maps of each whole utterance, built here in numpy: E' = |W| (*) E + 1e-5 S
    through a convolution (S = sum |terms| + |b|), the window maximum of E
    through a pool, unchanged through a ReLU; a frame's row of it is the
    gather of the maps.  S is taken on the fp64 maps, not on either pass's own
    values, which moves it by E / S ~ 1e-5 of itself: 0.1 % is added for that;
  * the results differ by at most the bound test_gpu_online.py holds a stream
    to against Compute: RTOL x conv_net_error_scale for nets A and B; for S
    and P, whose layers above the prefix are an FC and the Softmax, the same
    derivation from E (result_error_scale's FC and Softmax steps).
With integer data (check 3 of test_gpu_compute_shared.py) the two computers'
results are bit-identical through the whole schedule and Output(prefix - 1)
equals the oracle's window pass.

Then the fallbacks (a Splice above component 0, the literal path: today's
Accept bit for bit), the state a computer keeps (none more than before), and
nnet.config's test model."""
import numpy as np
import pytest

from _util import assert_same, dev, host, rng
from test_gpu_compute import RTOL, net_of, nnet_config_model, utterances, windows
from test_gpu_compute_shared import (INPUT_RANGE, PREFIX, config_lines, integer_net, line_args,
                                     oracle_prefix, shared_net, taps)
from test_gpu_online import (LENGTHS, MAX_CHUNK, SCHEDULE, SEED, STREAMS, Model,
                             conv_net_error_scale, results_equal, run_steps)

pytestmark = pytest.mark.gpu
F32 = np.float32


def pair(kc, net, lengths=LENGTHS, **kw):
    """(default computer, its model, shared computer, its model) on one net."""
    own = kc.OnlineComputer(net, STREAMS, MAX_CHUNK, **kw)
    shared = kc.OnlineComputer(net, STREAMS, MAX_CHUNK, share_time=True, **kw)
    right = net.RightContext()
    return own, Model(right, lengths), shared, Model(right, lengths)


def truth_maps(net, name, prefix, x):
    """The gathered last time map of one whole utterance in fp64, [T x C n],
    and the bar E at each of its elements."""
    left, right = net.LeftContext(), net.RightContext()
    t_len = len(x)
    args = [line_args(ln) for ln in config_lines(name)]
    kinds = [c.Type() for c in net.components]
    cur = x[np.clip(np.arange(-left, t_len + right), 0, t_len - 1)].astype(np.float64)
    err = np.zeros_like(cur)
    n, delta = left + right + 1, 1
    for lvl in range(1, prefix):
        if kinds[lvl] == "ConvolutionComponent":
            ws, b = taps(net.components[lvl], kinds[lvl - 1], cur.shape[1])
            rows = cur.shape[0] - delta * (len(ws) - 1)
            t = np.tile(b.astype(np.float64), (rows, 1))
            s, e = np.abs(t), np.zeros_like(t)
            for k, w in enumerate(ws):
                w64 = w.astype(np.float64)
                a = cur[delta * k:delta * k + rows]
                t += a @ w64
                s += np.abs(a) @ np.abs(w64)
                e += err[delta * k:delta * k + rows] @ np.abs(w64)
            cur, err, n = t, e + RTOL * s * 1.001, n - len(ws) + 1
        elif kinds[lvl] == "MaxpoolComponent":
            pw, pc = args[lvl]["pool-width-dim"], args[lvl]["pool-channel-dim"]
            rows = cur.shape[0] - delta * (pw - 1)
            pick = [(w, c) for c in range(pc) for w in range(pw)]
            cur = np.max([cur[delta * w:delta * w + rows][:, c::pc] for w, c in pick], axis=0)
            err = np.max([err[delta * w:delta * w + rows][:, c::pc] for w, c in pick], axis=0)
            assert cur.min() > -1e20
            n, delta = n // pw, delta * pw
        else:
            assert kinds[lvl] == "RectifiedLinearComponent"
            cur = np.maximum(cur, 0.0)

    def gather(m):
        out = np.empty((t_len, m.shape[1] * n))
        for k in range(n):
            out[:, k::n] = m[delta * k:delta * k + t_len]
        return out
    assert cur.shape[0] >= t_len + delta * (n - 1)
    return gather(cur), gather(err)


def upper_scale(net, prefix, top, top_err):
    """From the bar E of Output(prefix - 1) (`top`: its fp64 values) to an
    absolute bound on the difference of two results, for a net whose components
    above the prefix are FC, ReLU and a last Softmax, as result_error_scale of
    test_gpu_compute.py derives it: an FC adds RTOL x its own S and passes E on
    through |W|; ReLU does not grow it; |dP| <= 2 P max |dx| through the Softmax
    (1e-6 P more for the kernel's own roundings of exp and the division); two
    such results differ by twice that."""
    x, err = top, top_err
    for comp in net.components[prefix:]:
        kind = comp.Type()
        if kind == "FullyConnectedComponent":
            w, b = host(comp.LinearParams()).astype(np.float64), host(comp.BiasParams())
            s = np.abs(x) @ np.abs(w).T + np.abs(b)
            x, err = x @ w.T + b, RTOL * s * 1.001 + err @ np.abs(w).T
        elif kind == "RectifiedLinearComponent":
            x = np.maximum(x, 0.0)
        else:
            assert kind == "SoftmaxComponent" and comp is net.components[-1]
            p = np.exp(x - x.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            x, err = p, 2.0 * p * err.max(axis=1, keepdims=True) + 1e-6 * p
    return 2.0 * err


def check_pair(kc, name, net, utts, steps, what, lengths=LENGTHS):
    prefix = PREFIX[name]
    own, own_model, shared, shared_model = pair(kc, net, lengths)
    assert shared.TimeSharedPrefix() == prefix and own.TimeSharedPrefix() == 0
    truth = [truth_maps(net, name, prefix, x) for x in utts]
    if name in "AB":
        bound = []
        for x in utts:
            net.Compute(dev(x))
            bound.append(RTOL * conv_net_error_scale(net))
    else:
        bound = [upper_scale(net, prefix, t, e) for t, e in truth]
    quiet = 0
    for entries in steps:
        ((emitted, y),) = run_steps(shared, shared_model, utts, (entries,))
        if emitted:
            top = host(net.Output(prefix - 1)).copy()
            for i in range(prefix - 1):
                with pytest.raises(kc.KcnnError, match="time maps"):
                    net.Output(i)
        ((emitted_own, y_own),) = run_steps(own, own_model, utts, (entries,))
        assert emitted == emitted_own and y.shape == y_own.shape
        if not emitted:
            quiet += 1
            continue
        top_own = host(net.Output(prefix - 1)).copy()
        bar = 2.0 * np.stack([truth[u][1][t] for u, t in emitted])
        diff = np.abs(top.astype(np.float64) - top_own)
        print(f"{what} {entries}: worst |shared - own| / 2E = "
              f"{(diff / np.maximum(bar, 1e-300)).max():.3e}")
        assert top.shape == bar.shape and (diff <= bar).all(), \
            f"{what}: {(diff > bar).sum()} elements of Output({prefix - 1}) differ by more than 2 E"
        lim = np.stack([bound[u][t] for u, t in emitted])
        diff = np.abs(y.astype(np.float64) - y_own)
        print(f"{what} {entries}: worst result difference / bound = "
              f"{(diff / np.maximum(lim, 1e-300)).max():.3e}")
        assert np.isfinite(y).all() and (diff <= lim + 1e-30).all(), \
            f"{what}: {(diff > lim).sum()} elements of the result outside the bound"
    assert quiet >= 1 and not shared_model.slots and not own_model.slots


@pytest.mark.parametrize("name", ["A", "B", "S", "P"])
def test_against_the_default_computer(kc, name):
    net = shared_net(name)
    utts = utterances(LENGTHS, net.components[0].InputDim(), SEED)
    check_pair(kc, name, net, utts, SCHEDULE, f"net {name}")


@pytest.mark.parametrize("name", ["A", "B", "S", "P"])
def test_integer_data_is_exact_and_bit_identical(kc, name):
    net = integer_net(name)
    prefix = PREFIX[name]
    left, right = net.LeftContext(), net.RightContext()
    d = net.components[0].InputDim()
    r = rng(5700 + ord(name))
    utts = [r.integers(-INPUT_RANGE, INPUT_RANGE + 1, size=(t, d)).astype(F32) for t in LENGTHS]
    win = windows(utts, left, right).reshape(sum(LENGTHS), -1)
    want, biggest = oracle_prefix(name, net, prefix, np.ascontiguousarray(win))
    assert biggest < 2 ** 11 and (want == np.round(want)).all()
    first = np.concatenate([[0], np.cumsum(LENGTHS)])
    priors = (rng(5701).random(net.components[-1].OutputDim()) + 0.01).astype(F32)
    for kw in ({}, {"apply_log": True, "priors": priors, "prior_scale": 0.5}):
        own, own_model, shared, shared_model = pair(kc, net, **kw)
        assert shared.TimeSharedPrefix() == prefix
        for entries in SCHEDULE:
            ((emitted, y),) = run_steps(shared, shared_model, utts, (entries,))
            top = host(net.Output(prefix - 1)).copy() if emitted else None
            ((_, y_own),) = run_steps(own, own_model, utts, (entries,))
            assert_same(y, y_own, f"net {name} {sorted(kw)}: the result of {entries}")
            if emitted:
                rows = [first[u] + t for u, t in emitted]
                assert_same(top, want[rows], f"net {name}: Output({prefix - 1}) of {entries}")
                assert_same(host(net.Output(prefix - 1)), want[rows], f"net {name}: the default's")


# ---- fallbacks ----------------------------------------------------------------------------
def bits_through_the_schedule(kc, net, utts, what):
    own, own_model, shared, shared_model = pair(kc, net)
    assert shared.TimeSharedPrefix() == 0
    results_equal(run_steps(shared, shared_model, utts, SCHEDULE),
                  run_steps(own, own_model, utts, SCHEDULE), what)


@pytest.mark.parametrize("name", ["D", "E"])
def test_a_splice_above_component_0_is_todays_accept(kc, name):
    net = net_of(name)
    bits_through_the_schedule(kc, net, utterances(LENGTHS, net.components[0].InputDim(), SEED),
                              f"net {name}")


@pytest.mark.parametrize("name", ["B", "S"])
def test_the_literal_path_is_todays_accept(kc, name):
    net = shared_net(name)
    try:
        kc.set_literal_path(True)
        bits_through_the_schedule(kc, net, utterances(LENGTHS, 8, SEED), f"net {name}, literal")
    finally:
        kc.set_literal_path(False)


def test_toggling_the_literal_path_between_steps(kc):
    """A step takes either route whatever the last one took: every step gives
    the bits the same step gives in a run that never toggles."""
    net = shared_net("S")
    utts = utterances(LENGTHS, 8, SEED)
    _, _, shared, model = pair(kc, net)
    want_shared = run_steps(shared, model, utts, SCHEDULE)
    own, model, _, _ = pair(kc, net)
    try:
        kc.set_literal_path(True)
        want_literal = run_steps(own, model, utts, SCHEDULE)
        _, _, shared, model = pair(kc, net)
        for k, entries in enumerate(SCHEDULE):
            literal = k % 2 == 1
            kc.set_literal_path(literal)
            assert shared.TimeSharedPrefix() == (0 if literal else 8)
            got = run_steps(shared, model, utts, (entries,))
            results_equal(got, [(want_literal if literal else want_shared)[k]],
                          f"step {k}, literal {literal}")
    finally:
        kc.set_literal_path(False)


# ---- state ----------------------------------------------------------------------------------
def test_other_forward_calls_between_steps_change_no_later_row(kc):
    net = shared_net("S")
    utts = utterances(LENGTHS, 8, SEED)
    _, _, shared, model = pair(kc, net)
    want = run_steps(shared, model, utts, SCHEDULE)
    other = dev(rng(5800).standard_normal((11, 8)).astype(F32))
    win = dev(rng(5801).standard_normal((3 * 11, 8)).astype(F32))

    def between():
        net.Compute(other, [4, 7])
        net.Compute(other, [4, 7], share_time=True)
        net.Propagate(win)
    _, _, shared, model = pair(kc, net)
    results_equal(run_steps(shared, model, utts, SCHEDULE, between=between), want,
                  "with Compute, Compute(share_time=True) and Propagate between the steps")


def test_reset_mid_utterance_and_slot_reuse(kc):
    net = shared_net("B")
    utts = utterances(LENGTHS, 8, SEED)
    tail = (((1, 2, 8, False), (3, 1, 2, False)), ((3, 1, 3, True), (1, 2, 8, False)),
            ((1, 2, 8, False),), ((1, 2, 8, False),), ((1, 2, 5, True),))
    _, _, shared, model = pair(kc, net)
    want = run_steps(shared, model, utts, tail)
    _, _, shared, model = pair(kc, net)
    other = Model(net.RightContext(), LENGTHS)
    run_steps(shared, other, utts, (((1, 2, 8, False),), ((1, 2, 3, False),)), streams=0)
    assert shared.Frames(1) == (11, 9)
    shared.Reset(1)
    shared.Accept(dev(utts[2][:8]), [3], [8], [False])
    shared.Reset(3)
    assert shared.Frames(1) == shared.Frames(3) == (0, 0)
    results_equal(run_steps(shared, model, utts, tail), want, "slots reused after Reset")


def test_a_refused_step_launches_nothing_and_moves_no_slot(kc):
    net = shared_net("B")
    utts = utterances(LENGTHS, 8, SEED)
    head, rest = SCHEDULE[:4], SCHEDULE[4:]
    _, _, twin, twin_model = pair(kc, net)
    run_steps(twin, twin_model, utts, head)
    want = run_steps(twin, twin_model, utts, rest)
    _, _, shared, model = pair(kc, net)
    (*_, (_, last)) = run_steps(shared, model, utts, head)
    view, top = net.Output(), host(net.Output(3)).copy()
    frames = [shared.Frames(s) for s in range(STREAMS)]
    good = dev(np.zeros((3, 8), F32))
    for what, chunk, streams, num_new, final in (
            ("stream 4 outside", good, [2, 4], [2, 1], [False, False]),
            ("named twice", good, [2, 0, 2], [1, 1, 1], [False, False, True]),
            ("9 new frames outside", dev(np.zeros((9, 8), F32)), [2], [9], [False]),
            ("sum to 2, the chunk has 3", good, [2], [2], [True]),
            ("a chunk of 7 columns", dev(np.zeros((3, 7), F32)), [2], [3], [False])):
        with pytest.raises(kc.KcnnError, match=what):
            shared.Accept(chunk, streams, num_new, final)
        assert [shared.Frames(s) for s in range(STREAMS)] == frames, what
    assert_same(host(view), last, "the last result after the refused steps")
    assert_same(host(net.Output(3)), top, "the last gathered map after the refused steps")
    results_equal(run_steps(shared, model, utts, rest), want, "the steps after the refused ones")


@pytest.mark.parametrize("extra_cols", [3, 4])  # a chunk stride of 11 (scalar), of 12 (16-byte)
def test_strided_chunks(kc, extra_cols):
    net = shared_net("S")
    utts = utterances(LENGTHS, 8, SEED)
    _, _, shared, model = pair(kc, net)
    want = run_steps(shared, model, utts, SCHEDULE)
    _, _, shared, model = pair(kc, net)
    results_equal(run_steps(shared, model, utts, SCHEDULE, layout=extra_cols), want,
                  f"a chunk stride of {8 + extra_cols}")


def test_the_largest_step_after_the_smallest(kc):
    """The level maps are sized once, by the first accepted step, for the most
    rows a step can have: a step of one frame, then the largest step there is
    (every slot ends with max_chunk frames behind R waiting ones: max_chunk + L
    + 2 R map rows a slot), held to the bounds of the pair test."""
    net = shared_net("S")
    right = net.RightContext()
    n = right + MAX_CHUNK
    lengths = (n,) * STREAMS
    slots = list(range(STREAMS))
    steps = (tuple((s, s, 1, False) for s in slots[:1]),
             tuple((s, s, right if s else right - 1, False) for s in slots),
             tuple((s, s, MAX_CHUNK, True) for s in slots))
    check_pair(kc, "S", net, utterances(lengths, 8, SEED + 1), steps, "net S, largest step",
               lengths=lengths)


# ---- nnet.config's test model -----------------------------------------------------------
def test_nnet_config_model(kc):
    net = nnet_config_model()
    lengths = (9, 4, 6)
    utts = utterances(lengths, 40, 5900)
    own = kc.OnlineComputer(net, 3, 4)
    shared = kc.OnlineComputer(net, 3, 4, share_time=True)
    assert shared.TimeSharedPrefix() == 14 and own.TimeSharedPrefix() == 0
    steps = (((0, 0, 4, False), (1, 1, 4, True), (2, 2, 4, False)),
             ((2, 2, 2, False), (0, 0, 4, False)),
             ((0, 0, 1, True), (2, 2, 0, True)))
    truth = [truth_maps(net, "nnet", 14, x) for x in utts]
    bound = [upper_scale(net, 14, t, e) for t, e in truth]
    own_model, shared_model = Model(10, lengths), Model(10, lengths)
    emitted_rows = 0
    for entries in steps:
        ((emitted, y),) = run_steps(shared, shared_model, utts, (entries,), streams=3)
        top = host(net.Output(13)).copy() if emitted else None
        ((_, y_own),) = run_steps(own, own_model, utts, (entries,), streams=3)
        if not emitted:
            continue
        emitted_rows += len(emitted)
        bar = 2.0 * np.stack([truth[u][1][t] for u, t in emitted])
        diff = np.abs(top.astype(np.float64) - host(net.Output(13)))
        print(f"nnet.config {entries}: worst |shared - own| / 2E = "
              f"{(diff / np.maximum(bar, 1e-300)).max():.3e}")
        assert (diff <= bar).all()
        lim = np.stack([bound[u][t] for u, t in emitted])
        diff = np.abs(y.astype(np.float64) - y_own)
        print(f"nnet.config {entries}: worst result difference / bound = "
              f"{(diff / np.maximum(lim, 1e-300)).max():.3e}")
        assert y.shape[1] == 3454 and np.isfinite(y).all() and (diff <= lim + 1e-30).all()
    assert emitted_rows == sum(lengths) and not shared_model.slots
