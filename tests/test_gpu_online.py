"""OnlineComputer: the streaming forward pass over concurrent utterances, on
the GPU.

Yardstick.  A step of Accept emits some frames of some utterances.  The same
whole utterances are held by a kcnn.Corpus, and PropagateFrames (existing code)
runs on the corpus rows of the step's emitted frames in the step's row order:
rows and row count are then the same and the splice is a copy, so Accept
without apply_log must equal Output() BIT FOR BIT, in the fused and the literal
path and in fusion modes 1 and 2, for the nets A to E of test_gpu_compute.py.
What a step must emit -- which frames, of which slots, how many -- comes from a
model of the issue's semantics below (ready = seen if final else max(0, seen -
R)), not from the library.

Each utterance's concatenated rows are then checked against Compute on the
whole utterance under assert_bound at the FC bar (rtol 1e-5) with the error
scale of test_batch_against_single, since the row counts differ and the FC
GEMMs scale their operands per column of the whole matrix; for nets A and B,
whose Conv, Maxpool and Normalize layers that scale does not cover, it is
extended below (conv_net_error_scale).  Nets whose only Splice is component 0
are checked against Propagate on the numpy-built windows under the same bound.

The log-likelihood epilogue must equal, within 1 ulp of fp32, the fp64 formula
of test_loglikes applied to the host copy of the same step's P.
"""
import numpy as np
import pytest

from _util import assert_bound, assert_same, dev, host, padded, rng
from test_gpu_compute import (CONFIGS, RTOL, assert_within_one_ulp, expected_loglikes, net_of,
                              propagate_reference, result_error_scale, run_modes, utterances)

pytestmark = pytest.mark.gpu

F32 = np.float32
STREAMS, MAX_CHUNK = 4, 8
LENGTHS = (1, 5, 37, 2, 3)  # L = R = 2: T = 1, L + R + 1, 37, 2 = L, 3
SEED = 5100
# (slot, utterance, new frames, final) per named slot and step.  Slots 0, 1, 2
# run utterances 0, 1, 2 interleaved; slot 0 is reused for utterances 3 and 4.
SCHEDULE = (
    # T = 1 ended in its first step; a first chunk shorter than R + 1 (slot 1
    # emits nothing); a chunk of exactly max_chunk
    ((0, 0, 1, True), (1, 1, 1, False), (2, 2, 8, False)),
    ((0, 3, 2, True),),                   # T = 2 = L ended in its first step, alone
    ((0, 4, 1, False),),                  # no slot emits: [0 x OutputDim]
    ((2, 2, 8, False), (0, 4, 1, False), (1, 1, 4, True)),  # another order; final with frames
    ((0, 4, 1, False), (2, 2, 1, False)),                   # one frame a step
    ((2, 2, 8, False), (0, 4, 0, True)),                    # final alone, beside another slot
    ((2, 2, 8, False),),
    ((2, 2, 3, False),),
    ((2, 2, 1, False),),
    ((2, 2, 0, True),),                                     # final alone, alone
)


class Model:
    """The issue's semantics on the host: what each step's chunk holds and
    which (utterance, frame) rows it must emit, in order."""

    def __init__(self, right, lengths):
        self.right, self.lengths = right, lengths
        self.slots = {}  # slot -> [utterance, seen, emitted]

    def frames(self, slot):
        return tuple(self.slots.get(slot, [None, 0, 0])[1:])

    def step(self, entries):
        chunk, emitted, counts = [], [], []
        for slot, u, n, final in entries:
            st = self.slots.setdefault(slot, [u, 0, 0])
            if st[1] == 0:
                st[0] = u
            assert st[0] == u, "the schedule mixes utterances in a slot"
            chunk += [(u, st[1] + k) for k in range(n)]
            st[1] += n
            ready = st[1] if final else max(0, st[1] - self.right)
            emitted += [(u, t) for t in range(st[2], ready)]
            counts.append(ready - st[2])
            st[2] = ready
            if final:
                assert st[1] == self.lengths[u], "the schedule ends an utterance short"
                del self.slots[slot]
        return chunk, emitted, counts


def run_steps(oc, model, utts, steps, layout="contiguous", between=None, streams=STREAMS):
    """Feeds the steps; returns per step (emitted (utterance, frame) list,
    host copy of the result).  Counts and Frames are checked against the model."""
    results = []
    for entries in steps:
        chunk, emitted, counts = model.step(entries)
        x = None
        if chunk:
            rows = np.stack([utts[u][t] for u, t in chunk])
            x = dev(rows) if layout == "contiguous" else padded(rows, layout)
        out, got = oc.Accept(x, [e[0] for e in entries], [e[2] for e in entries],
                             [e[3] for e in entries])
        y = host(out).copy()
        assert got == counts, (entries, got, counts)
        assert y.shape[0] == len(emitted), (entries, y.shape)
        for s in range(streams):
            assert oc.Frames(s) == model.frames(s), (entries, s)
        results.append((emitted, y))
        if between is not None:
            between()
    return results


def fresh(kc, net, **kw):
    """A new computer on `net` and the model of its slots."""
    oc = kc.OnlineComputer(net, kw.pop("num_streams", STREAMS), kw.pop("max_chunk", MAX_CHUNK),
                           **kw)
    return oc, Model(net.RightContext(), LENGTHS)


def corpus_of(kc, utts):
    starts = np.concatenate([[0], np.cumsum([len(u) for u in utts])])
    return kc.Corpus(dev(np.concatenate(utts)), [len(u) for u in utts]), starts


def check_against_propagate_frames(kc, name, layout="contiguous"):
    net = net_of(name)
    utts = utterances(LENGTHS, net.components[0].InputDim(), SEED)
    corpus, starts = corpus_of(kc, utts)
    oc, model = fresh(kc, net)
    quiet = 0
    for emitted, y in run_steps(oc, model, utts, SCHEDULE, layout):
        assert y.shape[1] == net.components[-1].OutputDim()
        if not emitted:
            quiet += 1
            continue
        # (a forward call of the net between two steps, too)
        net.PropagateFrames(corpus, [starts[u] + t for u, t in emitted])
        assert_same(y, host(net.Output()), f"net {name}, the step emitting {emitted[:3]}..")
    assert quiet >= 1, "the schedule has a step in which no slot emits"
    assert not model.slots, "every utterance ended"


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_each_step_is_propagate_frames_on_its_rows(kc, name):
    run_modes(kc, lambda: check_against_propagate_frames(kc, name))


def by_utterance(results):
    """Each utterance's rows over the steps, which must be its frames in order."""
    rows = {}
    for emitted, y in results:
        for (u, t), row in zip(emitted, y):
            assert t == len(rows.setdefault(u, [])), f"utterance {u}: frame {t} out of order"
            rows[u].append(row)
    return {u: np.stack(r) for u, r in rows.items()}


def conv_net_error_scale(net):
    """result_error_scale for nets A and B (conv_net(d): Splice, Conv, Maxpool,
    ReLU, Normalize, FC, Softmax), from the activations the last Compute on
    one padded utterance left: S such that two results whose GEMM layers each
    hold the 1e-5·S bar differ by at most RTOL * S.  `err` is a bound on an
    activation's error in units of RTOL.  The Splice copies exact input.  A
    Conv or FC adds its own S (the oracle's third mode) and passes err on
    through |W|.  |max a - max b| <= max |a - b|, so the pool takes the
    window's largest err; ReLU does not grow it.  Normalize, y = x / rms(x):
    |rms(x + e) - rms(x)| <= |e|_2 / sqrt(D), hence |dy_i| <= e_i / rms + |x_i|
    |e|_2 / (sqrt(D) rms^2) to first order; 1 % is added for the higher orders
    (err is of the order of 1e-5 |x|) and 0.1 |y| (1e-6 relative) for the
    kernel's own roundings.  Softmax and the factor 2 as in
    result_error_scale."""
    import oracle as O
    from _util import triple
    d = net.components[0].InputDim()
    err = None
    for i, comp in enumerate(net.components):
        kind = comp.Type()
        x = host(net.Output(i - 1)).copy()
        if kind == "SpliceComponent":
            assert i == 0
            err = np.zeros((x.shape[0], comp.OutputDim()))
        elif kind in ("ConvolutionComponent", "FullyConnectedComponent"):
            if kind == "ConvolutionComponent":
                own, mag = O.Conv(d, 5, 1, d, 2, 4), O.Conv(d, 5, 1, d, 2, 4)
            else:
                own, mag = (O.FC(comp.InputDim(), comp.OutputDim()) for _ in range(2))
            own.W, own.b = host(comp.LinearParams()), host(comp.BiasParams())
            mag.W, mag.b = np.abs(own.W), np.zeros_like(own.b)
            _, _, s = triple(lambda: own.propagate(x))
            with O.accum(1):
                passed = mag.propagate(np.ascontiguousarray(err, F32))
            err = s.astype(np.float64) + passed.astype(np.float64) * (1 + 1e-6)
        elif kind == "MaxpoolComponent":
            err = O.Pool(1, 4, 4, 1, 2, 1).propagate(np.ascontiguousarray(err, F32)) \
                .astype(np.float64) * (1 + 1e-6)
        elif kind == "NormalizeComponent":
            x64 = x.astype(np.float64)
            rms = np.sqrt((x64 * x64).mean(axis=1, keepdims=True))
            assert (rms > 1e-3).all(), "a row near the floor: the bound does not hold there"
            e2 = np.sqrt((err * err).sum(axis=1, keepdims=True))
            err = 1.01 * (err / rms + np.abs(x64) * e2 / (np.sqrt(x.shape[1]) * rms * rms)) \
                + 0.1 * np.abs(x64) / rms
        elif kind == "SoftmaxComponent":
            p = host(net.Output(i)).astype(np.float64)
            err = 2.0 * p * err.max(axis=1, keepdims=True)
        else:
            assert kind == "RectifiedLinearComponent", kind
    return 2.0 * err


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_streams_against_whole_utterances(kc, name):
    net = net_of(name)
    utts = utterances(LENGTHS, net.components[0].InputDim(), SEED)
    oc, model = fresh(kc, net)
    got = by_utterance(run_steps(oc, model, utts, SCHEDULE))
    scales = []
    for u, x in enumerate(utts):
        whole = host(net.Compute(dev(x))).copy()
        scales.append(conv_net_error_scale(net) if name in "AB"
                      else result_error_scale(net, (len(x),)))
        assert got[u].shape == whole.shape == (len(x), whole.shape[1])
        print(f"net {name} utterance {u}: worst |stream - whole| / S = "
              f"{(np.abs(got[u].astype(np.float64) - whole) / scales[-1]).max():.3e}")
        assert_bound(got[u], whole, scales[-1], rtol=RTOL, what=f"net {name} utterance {u}")
    if name in "ABC":  # the only Splice is component 0: Propagate on the windows
        want = propagate_reference(name, LENGTHS, SEED, False, 1)
        assert_bound(np.concatenate([got[u] for u in range(len(utts))]), want,
                     np.concatenate(scales), rtol=RTOL, what=f"net {name} against Propagate")


# ---- layouts --------------------------------------------------------------------------
@pytest.mark.parametrize("name, extra_cols", [("B", 3), ("B", 4), ("A", 3), ("C", 4)])
def test_strided_chunk(kc, name, extra_cols):
    """Net B: a chunk stride of 11 (scalar accesses) and of 12 (16-byte); net
    A's 5 columns are scalar either way; net C has the const-component tail."""
    check_against_propagate_frames(kc, name, layout=extra_cols)


@pytest.mark.parametrize("d", [513, 2052])  # scalar; 16-byte accesses
def test_more_row_groups_than_blocks(kc, d):
    """Rows this wide make every written row a group of its own, and a step of
    16 slots x 70 frames writes more groups than the assembly kernel's grid has
    blocks (1024): the blocks' stride over the groups.  The second step moves
    tails out of the arena too.  A Splice alone, against numpy indexing."""
    net = kc.Nnet(f"SpliceComponent input-dim={d} left-context=2 right-context=2 "
                  "const-component-dim=0")
    n, t = 16, 140
    x = rng(5200).standard_normal((n, t, d)).astype(F32)
    oc = kc.OnlineComputer(net, n, 70)
    idx = np.clip(np.arange(t)[:, None] + np.arange(-2, 3)[None, :], 0, t - 1)
    want = x[:, idx].reshape(n, t, 5 * d)
    slots = list(range(n))
    out, counts = oc.Accept(dev(x[:, :70].reshape(n * 70, d)), slots, [70] * n, [False] * n)
    assert counts == [68] * n
    assert_same(host(out), want[:, :68].reshape(n * 68, 5 * d), f"dim {d}, step 1")
    out, counts = oc.Accept(dev(x[:, 70:].reshape(n * 70, d)), slots, [70] * n, [True] * n)
    assert counts == [72] * n
    assert_same(host(out), want[:, 68:].reshape(n * 72, 5 * d), f"dim {d}, step 2")


# ---- state ----------------------------------------------------------------------------
def results_equal(a, b, what):
    assert len(a) == len(b)
    for (ea, ya), (eb, yb) in zip(a, b):
        assert ea == eb
        assert_same(ya, yb, what)


@pytest.mark.parametrize("how", ["final", "reset"])
def test_a_reused_slot_holds_no_stale_history(kc, how):
    net = net_of("B")
    utts = utterances(LENGTHS, 8, SEED)
    tail = (((1, 2, 8, False), (3, 1, 2, False)), ((3, 1, 3, True), (1, 2, 8, False)),
            ((1, 2, 8, False),), ((1, 2, 8, False),), ((1, 2, 5, True),))
    oc, model = fresh(kc, net)
    want = run_steps(oc, model, utts, tail)
    oc, model = fresh(kc, net)
    if how == "final":
        run_steps(oc, model, utts, (((1, 1, 3, False), (3, 4, 3, False)),
                                    ((1, 1, 2, True), (3, 4, 0, True))))
    else:
        # another history in slots 1 and 3 (37 frames, of which 11 and 8 are in), abandoned
        other = Model(net.RightContext(), LENGTHS)
        run_steps(oc, other, utts, (((1, 2, 8, False),), ((1, 2, 3, False),)), streams=0)
        assert oc.Frames(1) == (11, 9)
        oc.Reset(1)
        oc.Accept(dev(utts[2][:8]), [3], [8], [False])
        oc.Reset(3)
        assert oc.Frames(1) == oc.Frames(3) == (0, 0)
    results_equal(run_steps(oc, model, utts, tail), want, f"slots reused after {how}")


def test_other_forward_calls_between_steps_disturb_nothing(kc):
    net = net_of("A")
    utts = utterances(LENGTHS, 5, SEED)
    oc, model = fresh(kc, net)
    want = run_steps(oc, model, utts, SCHEDULE)
    other = dev(rng(5300).standard_normal((11, 5)).astype(F32))
    windows = dev(rng(5301).standard_normal((3 * 5, 5)).astype(F32))

    def between():
        net.Compute(other, [4, 7])
        net.Propagate(windows)
    oc, model = fresh(kc, net)
    results_equal(run_steps(oc, model, utts, SCHEDULE, between=between), want,
                  "with Compute and Propagate between the steps")


def test_accept_leaves_the_inference_state(kc):
    kc.set_randn_seed(5400)
    net = kc.Nnet(CONFIGS["C"])
    oc = kc.OnlineComputer(net, 2, 4)
    x = dev(rng(5401).standard_normal((4, 6)).astype(F32))
    out, counts = oc.Accept(x, [1], [4], [True])
    assert counts == [4] and out.shape == (4, 9)
    with pytest.raises(kc.KcnnError, match="propagate first"):
        net.BackpropXent([(0, 0, 1.0)])
    assert_same(host(net.Output()), host(out), "the last output is the result")


# ---- the log-likelihood epilogue ---------------------------------------------------------
def loglike_runs(kc, net, utts, priors, prior_scale):
    """(P per step, log-likelihoods per step), two computers on one net."""
    ocp, mp = fresh(kc, net)
    ocl, ml = fresh(kc, net, priors=priors, prior_scale=prior_scale, apply_log=True)
    ps, lls = [], []
    for entries in SCHEDULE:
        (_, p), = run_steps(ocp, mp, utts, (entries,))
        (_, ll), = run_steps(ocl, ml, utts, (entries,))
        ps.append(p)
        lls.append(ll)
    return ps, lls


@pytest.mark.parametrize("name", ["A", "D"])
def test_loglikes_of_each_step(kc, name):
    net = net_of(name)
    cols = net.components[-1].OutputDim()
    utts = utterances(LENGTHS, net.components[0].InputDim(), SEED)
    priors = (rng(5500).random(cols) + 0.01).astype(F32)
    got = {}
    try:
        for literal in (False, True):
            kc.set_literal_path(literal)
            got[literal] = loglike_runs(kc, net, utts, priors, 0.5)
    finally:
        kc.set_literal_path(False)
    for step, (p, ll) in enumerate(zip(*got[False])):
        assert ll.shape == p.shape
        if len(p):
            assert_within_one_ulp(ll, expected_loglikes(p, priors, 0.5), f"net {name} step {step}")
    for a, b in zip(got[False][1], got[True][1]):
        assert_same(a, b, "fused against literal")


def test_loglikes_of_a_network_without_softmax(kc):
    """The element-wise kernel alone, without priors: the last component is
    not a Softmax, and values under the floor are floored."""
    net = kc.Nnet("SpliceComponent input-dim=4 left-context=1 right-context=1 "
                  "const-component-dim=0\nRectifiedLinearComponent dim=12")
    x = rng(5600).standard_normal((9, 4)).astype(F32)
    ocp, ocl = kc.OnlineComputer(net, 1, 5), kc.OnlineComputer(net, 1, 5, apply_log=True)
    for lo, hi, final in ((0, 5, False), (5, 9, True)):
        p = host(ocp.Accept(dev(x[lo:hi]), [0], [hi - lo], [final])[0]).copy()
        ll = host(ocl.Accept(dev(x[lo:hi]), [0], [hi - lo], [final])[0]).copy()
        assert (p == 0).any() and p.shape == (4 if not final else 5, 12)
        assert_within_one_ulp(ll, expected_loglikes(p), "ReLU network")


# ---- refusals on the device ------------------------------------------------------------
def test_refused_steps_change_nothing(kc):
    net = net_of("B")
    utts = utterances(LENGTHS, 8, SEED)
    head, rest = SCHEDULE[:4], SCHEDULE[4:]
    twin, twin_model = fresh(kc, net)
    run_steps(twin, twin_model, utts, head)
    want = run_steps(twin, twin_model, utts, rest)

    oc, model = fresh(kc, net)
    (*_, (_, last)) = run_steps(oc, model, utts, head)
    out, _ = oc.Accept(None, [], [], [])  # names no slot: nothing runs
    assert out.shape == (0, 12)
    view = net.Output()
    frames = [oc.Frames(s) for s in range(STREAMS)]
    assert frames[2] == (16, 14) and frames[0] == (2, 0)
    good = dev(np.zeros((3, 8), F32))
    for what, chunk, streams, num_new, final in (
            ("stream 4 outside", good, [2, 4], [2, 1], [False, False]),
            ("stream -1 outside", good, [-1], [3], [False]),
            ("named twice", good, [2, 0, 2], [1, 1, 1], [False, False, True]),
            ("9 new frames outside", dev(np.zeros((9, 8), F32)), [2], [9], [False]),
            ("-1 new frames outside", None, [2], [-1], [True]),
            ("no new frames for stream 0", good, [2, 0], [3, 0], [False, False]),
            ("sum to 2, the chunk has 3", good, [2], [2], [True]),
            ("sum to 4, the chunk has 3", good, [2, 0], [3, 1], [True, True]),
            ("a chunk of 7 columns", dev(np.zeros((3, 7), F32)), [2], [3], [False]),
            ("sum to 3, the chunk has 0", None, [2], [3], [False]),
    ):
        with pytest.raises(kc.KcnnError, match=what):
            oc.Accept(chunk, streams, num_new, final)
        assert [oc.Frames(s) for s in range(STREAMS)] == frames, what
    for s in (-1, STREAMS):
        with pytest.raises(kc.KcnnError, match="outside"):
            oc.Reset(s)
        with pytest.raises(kc.KcnnError, match="outside"):
            oc.Frames(s)
    for kw, what in (({"num_streams": 0}, "num_streams 0"), ({"max_chunk": 0}, "max_chunk 0"),
                     ({"priors": np.full(12, 0.1, F32)}, "apply_log"),
                     ({"priors": np.full(11, 0.1, F32), "apply_log": True}, "11 priors for 12")):
        with pytest.raises(kc.KcnnError, match=what):
            fresh(kc, net, **kw)
    assert_same(host(view), last, "the last result after the refused steps")
    results_equal(run_steps(oc, model, utts, rest), want, "the steps after the refused ones")
