"""Training from a device-resident corpus: Nnet.PropagateFrames /
ComputeProbFrames on minibatches given as corpus row indices, kcnn.Corpus and
kcnn.train_epoch, on the GPU.

Yardstick: existing code.  A twin network (Nnet.Copy: identical parameters,
momentum buffers and statistics; DropoutComponents given the same seed) runs
Propagate on the window matrix of the examples, built here in numpy from the
frame list: example n with corpus row r in the utterance of rows [s, e) is the
rows clamp(r + o, s, e - 1), o = -L .. R.  Both networks then run the same
kernels on equal inputs in one process, so every comparison is of BITS: every
Output(i), every parameter and PrevGrad, the NonlinearComponent statistics,
ObjfTotal / ProbTotal and the input derivatives.  No tolerance applies
anywhere in this file.
"""
import functools
import os

import numpy as np
import pytest

from _util import dev, host, padded, rng
from test_gpu_compute import (CONFIGS, F32, net_of, run_modes, snapshot, assert_unchanged,
                              utterances, windows)
from test_gpu_nnet import STACKS, build as build_stack

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = [(1, 7, 23, 2), (5,)]  # utterances of 1 and 2 frames: shorter than every context


def assert_bits(a, b, what):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = a.view(np.int32) != b.view(np.int32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ in bits"


def example_windows(utts, frames, left, right):
    """The matrix Propagate takes for the examples `frames` (corpus rows): the
    rows of windows() of their frames, in the examples' order."""
    win = windows(utts, left, right)
    cs = left + right + 1
    rows = (np.asarray(frames, np.int64)[:, None] * cs + np.arange(cs)[None, :]).ravel()
    return win[rows]


def frame_lists(lengths, seed):
    """Every corpus row, shuffled, with rows repeated up to 70 examples or
    more (more than one row group of the kernel); one example; the first and
    last row of each utterance only."""
    r = rng(seed)
    total = sum(lengths)
    many = np.concatenate([r.permutation(total), r.integers(0, total, size=max(5, 72 - total))])
    r.shuffle(many)
    assert len(many) >= 70 and set(many.tolist()) == set(range(total))
    ends, s = [], 0
    for t in lengths:
        ends += [s, s + t - 1]
        s += t
    return {"many": many.astype(np.int32), "one": np.asarray([total // 2], np.int32),
            "ends": np.asarray(ends, np.int32)}


@functools.lru_cache(maxsize=None)
def twin_of(name):
    return net_of(name).Copy()


def outputs(net):
    return [host(net.Output(i)).copy() for i in range(net.NumComponents())]


def check_forward(kc, net, twin, utts, lengths, frames, what, layout="contiguous"):
    left, right = net.LeftContext(), net.RightContext()
    stacked = np.concatenate(utts)
    x = dev(stacked) if layout == "contiguous" else padded(stacked, layout)
    corpus = kc.Corpus(x, list(lengths))
    win = example_windows(utts, frames, left, right)
    dwin = dev(win)
    splice_first = net.components[0].Type() == "SpliceComponent"

    def both():
        net.PropagateFrames(corpus, frames)
        got = outputs(net)
        first_input = host(net.Output(-1)).copy()
        twin.Propagate(dwin)
        return got, outputs(twin), first_input
    for mode, (got, want, first_input) in run_modes(kc, both).items():
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape[0] == len(frames) * (w.shape[0] // len(frames))
            assert_bits(g, w, f"{what} literal, fusion = {mode} Output({i})")
        # Output(-1): the borrowed corpus, or the window matrix laid out
        assert_bits(first_input, stacked if splice_first else win, f"{what} {mode} Output(-1)")


@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_forward_is_propagate_on_the_windows(kc, name, lengths):
    """A: scalar accesses (d = 5); B: 16-byte (d = 8); C: the const tail; D:
    gapped output offsets; E: component 0 a ReLU, the window matrix laid out."""
    net, twin = net_of(name), twin_of(name)
    utts = utterances(lengths, net.components[0].InputDim(), 1000 + len(lengths))
    for kind, frames in frame_lists(lengths, 1100).items():
        check_forward(kc, net, twin, utts, lengths, frames, f"net {name} {lengths} {kind}")


@pytest.mark.parametrize("extra_cols", [3, 4])  # net B: a stride of 11 (scalar), of 12 (16-byte)
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_strided_corpus(kc, name, extra_cols):
    net, twin = net_of(name), twin_of(name)
    lengths = LENGTHS[0]
    utts = utterances(lengths, net.components[0].InputDim(), 1200)
    frames = frame_lists(lengths, 1201)["many"]
    check_forward(kc, net, twin, utts, lengths, frames, f"net {name} stride + {extra_cols}",
                  layout=extra_cols)


def test_zero_context_stack_is_a_row_gather(kc):
    """Conv -> Maxpool -> FC (c2 of test_gpu_nnet.py) at 37 frames: the input
    chunk is one row, the pass before component 0 a plain row gather."""
    net = build_stack(kc, STACKS["c2"], seed=11)
    twin = net.Copy()
    assert (net.LeftContext(), net.RightContext()) == (0, 0)
    lengths = (10, 1, 26)
    utts = utterances(lengths, net.components[0].InputDim(), 1300)
    frames = rng(1301).permutation(37).astype(np.int32)
    check_forward(kc, net, twin, utts, lengths, frames, "c2 stack")


@pytest.mark.parametrize("d", [205, 820])  # 1025 columns (scalar), 4100 (16-byte accesses)
def test_more_row_groups_than_blocks(kc, d):
    """Rows this wide make every output row a group of its own, and 8300
    examples are more groups than the grid has blocks (8192): the blocks'
    stride over the groups, which no smaller shape reaches.  A Splice alone,
    against numpy indexing."""
    net = kc.Nnet(f"SpliceComponent input-dim={d} left-context=2 right-context=2 "
                  "const-component-dim=0")
    lengths = (1, 40, 2, 57)
    x = rng(1350).standard_normal((sum(lengths), d)).astype(F32)
    frames = rng(1351).integers(0, sum(lengths), size=8300).astype(np.int32)
    starts = np.cumsum((0,) + lengths)
    utt = np.searchsorted(starts, frames, side="right") - 1
    idx = np.clip(frames[:, None] + np.arange(-2, 3)[None, :], starts[utt][:, None],
                  starts[utt + 1][:, None] - 1)
    net.PropagateFrames(kc.Corpus(dev(x), list(lengths)), frames)
    assert_bits(host(net.Output()), x[idx].reshape(len(frames), 5 * d), f"dim {d}")


# ---- one training step ------------------------------------------------------------------
def sparse_labels(num_rows, num_cols):
    """Two labels on every third row, one on the next, none on the third."""
    out = []
    for n in range(num_rows):
        if n % 3 == 0:
            c = (5 * n) % num_cols
            out += [(n, min(c, (c + 3) % num_cols), 0.75), (n, max(c, (c + 3) % num_cols), 0.25)]
        elif n % 3 == 1:
            out.append((n, (7 * n) % num_cols, 1.0))
    return out


def seed_dropout(nets, seed):
    for net in nets:
        for k, c in enumerate(net.components):
            if c.Type() == "DropoutComponent":
                c.SetDropoutSeed(seed + k)


def assert_same_state(kc, net, twin, what):
    a, b = snapshot(net), snapshot(twin)
    assert len(a[0]) == len(b[0]) and len(a[1]) == len(b[1])
    for k, (p, q) in enumerate(zip(a[0], b[0])):
        assert_bits(host(p), host(q), f"{what}: parameter block {k}")
    for (v0, d0, c0), (v1, d1, c1) in zip(a[1], b[1]):
        np.testing.assert_array_equal(v0, v1)
        np.testing.assert_array_equal(d0, d1)
        assert c0 == c1
    assert net.ObjfTotal() == twin.ObjfTotal(), what


def check_step(kc, base, utts, lengths, frames, what):
    """PropagateFrames + BackpropXent on a copy of `base` against Propagate +
    BackpropXent on another, in the mode that is set."""
    net, twin = base.Copy(), base.Copy()
    seed_dropout((net, twin), 77)
    corpus = kc.Corpus(dev(np.concatenate(utts)), list(lengths))
    win = dev(example_windows(utts, frames, net.LeftContext(), net.RightContext()))
    labels = sparse_labels(len(frames), net.components[-1].OutputDim())
    net.PropagateFrames(corpus, frames)
    twin.Propagate(win)
    for i, (g, w) in enumerate(zip(outputs(net), outputs(twin))):
        assert_bits(g, w, f"{what}: Output({i})")
    net.BackpropXent(labels)
    twin.BackpropXent(labels)
    assert_same_state(kc, net, twin, what)
    assert net.ObjfTotal()[1] == sum(w for _, _, w in labels) > 0
    first = 0
    if net.components[0].Type() == "SpliceComponent":
        with pytest.raises(kc.KcnnError, match="SpliceComponent reads the corpus"):
            net.InputDeriv(0)
        first = 1
    for i in range(first, net.NumComponents()):
        assert_bits(host(net.InputDeriv(i)), host(twin.InputDeriv(i)), f"{what}: InputDeriv({i})")
    return net, twin


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_one_training_step(kc, name):
    lengths = LENGTHS[0]
    kc.set_randn_seed(4200 + ord(name))
    base = kc.Nnet(CONFIGS[name])
    utts = utterances(lengths, base.components[0].InputDim(), 1400)
    frames = frame_lists(lengths, 1401)["many"]
    for mode, (net, twin) in run_modes(
            kc, lambda: check_step(kc, base, utts, lengths, frames, f"net {name}")).items():
        if name == "E":  # component 0 ran its Backprop, over the laid-out matrix
            assert net.components[0].NonlinearStats()[2] == twin.components[0].NonlinearStats()[2] > 0
            assert net.InputDeriv(0).shape == (len(frames) * 5, 4)
        # a second step on the same networks: a Propagate after PropagateFrames
        # backpropagates through component 0 again
        win = dev(example_windows(utts, frames[:9], net.LeftContext(), net.RightContext()))
        net.Propagate(win)
        twin.Propagate(win)
        labels = sparse_labels(9, net.components[-1].OutputDim())
        net.BackpropXent(labels)
        twin.BackpropXent(labels)
        assert_same_state(kc, net, twin, f"net {name} {mode} second step")
        assert_bits(host(net.InputDeriv(0)), host(twin.InputDeriv(0)), f"net {name} InputDeriv(0)")


def test_nnet_config_step_with_dropout(kc):
    """The reference's own network at 64 examples of three utterances, its
    DropoutComponents drawing masks (the same in both networks: same seed,
    same call count)."""
    kc.set_randn_seed(2029)
    base = kc.Nnet(open(os.path.join(GOLDEN, "nnet.config")).read())
    base.components[-2].PerturbParams(0.05)  # the last FC starts at zero
    lengths = (30, 3, 50)
    utts = utterances(lengths, 40, 1500)
    frames = rng(1501).integers(0, sum(lengths), size=64).astype(np.int32)
    frames[:4] = [0, 29, 30, 82]
    net, twin = check_step(kc, base, utts, lengths, frames, "nnet.config")
    drop = [i for i, c in enumerate(net.components) if c.Type() == "DropoutComponent"]
    assert len(drop) == 2
    for i in drop:  # masks were drawn
        y = host(net.Output(i))
        assert (y == 0).any() and (y != 0).any()


# ---- ComputeProbFrames ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "E"])
def test_compute_prob_frames(kc, name):
    lengths = LENGTHS[0]
    kc.set_randn_seed(4300 + ord(name))
    net = kc.Nnet(CONFIGS[name])
    twin = net.Copy()
    d = net.components[0].InputDim()
    utts = utterances(lengths, d, 1600)
    frames = frame_lists(lengths, 1601)["many"]
    stacked = dev(np.concatenate(utts))
    corpus = kc.Corpus(stacked, list(lengths))
    win = dev(example_windows(utts, frames, net.LeftContext(), net.RightContext()))
    labels = sparse_labels(len(frames), net.components[-1].OutputDim())
    # what the forward calls give on a network that never saw ComputeProbFrames
    twin.Propagate(win)
    want_prop = outputs(twin)
    want_compute = host(twin.Compute(stacked, list(lengths))).copy()
    before = snapshot(net)

    def totals():
        net.ComputeProbFrames(corpus, frames, labels)
        twin.ComputeProb(win, labels)
        for call in (lambda: net.BackpropXent(labels),
                     lambda: net.BackpropComponent(net.NumComponents() - 1, win)):
            with pytest.raises(kc.KcnnError, match="propagate first"):
                call()
        assert_bits(host(net.Output()), host(twin.Output()), "P after ComputeProbFrames")
        return net.ProbTotal(reset=True), twin.ProbTotal(reset=True)
    for mode, (got, want) in run_modes(kc, totals).items():
        assert got == want and got[1] > 0, (mode, got, want)
    assert_unchanged(before, snapshot(net))
    assert net.ObjfTotal() == (0.0, 0.0)
    # the next forward call of each kind behaves as if the call had not happened
    net.ComputeProbFrames(corpus, frames, labels)
    net.Propagate(win)
    for i, (g, w) in enumerate(zip(outputs(net), want_prop)):
        assert_bits(g, w, f"Propagate after ComputeProbFrames Output({i})")
    net.ComputeProbFrames(corpus, frames, labels)
    net.PropagateFrames(corpus, frames)
    for i, (g, w) in enumerate(zip(outputs(net), want_prop)):
        assert_bits(g, w, f"PropagateFrames after ComputeProbFrames Output({i})")
    net.ComputeProbFrames(corpus, frames, labels)
    assert_bits(host(net.Compute(stacked, list(lengths))), want_compute,
                "Compute after ComputeProbFrames")
    # and the network trains from the next PropagateFrames
    net.PropagateFrames(corpus, frames)
    twin.Propagate(win)
    net.BackpropXent(labels)
    twin.BackpropXent(labels)
    assert_same_state(kc, net, twin, "a step after ComputeProbFrames")


# ---- refusals -----------------------------------------------------------------------------
def test_refused_calls_change_nothing(kc):
    lengths = LENGTHS[0]
    kc.set_randn_seed(4400)
    net = kc.Nnet(CONFIGS["A"])
    utts = utterances(lengths, 5, 1700)
    total = sum(lengths)
    stacked = np.concatenate(utts)
    x = dev(stacked)
    corpus = kc.Corpus(x, list(lengths))
    frames = frame_lists(lengths, 1701)["many"]
    labels = sparse_labels(len(frames), 12)
    net.PropagateFrames(corpus, frames)  # a step first: nothing is zero
    net.BackpropXent(labels)
    net.ComputeProbFrames(corpus, frames, labels)
    net.PropagateFrames(corpus, frames)
    want = outputs(net)
    view = net.Output()
    before, totals = snapshot(net), (net.ObjfTotal(), net.ProbTotal())

    # the corpus: an utterance of length < 1, lengths that do not sum to the rows
    for bad in ([1, 7, 23, 2, 0], [1, 7, 23, 3, -1], [1, 7, 23], [1, 7, 23, 3], []):
        with pytest.raises(kc.KcnnError):
            kc.Corpus(x, bad)
    narrow = kc.Corpus(dev(stacked[:, :4]), list(lengths))  # 4 columns for InputDim 5
    good = (0, 0, 1.0)
    for who in (lambda c, f: net.PropagateFrames(c, f),
                lambda c, f: net.ComputeProbFrames(c, f, [good])):
        for what, c, f in (("no frames", corpus, []), ("outside", corpus, [0, -1]),
                           ("outside", corpus, [0, total]),
                           ("outside", corpus, [2147483647]),
                           ("columns", narrow, [0])):
            with pytest.raises(kc.KcnnError, match=what):
                who(c, f)
    with pytest.raises(kc.KcnnError, match="outside"):  # a label past the examples
        net.ComputeProbFrames(corpus, frames[:3], [(3, 0, 1.0)])
    assert_unchanged(before, snapshot(net))
    assert (net.ObjfTotal(), net.ProbTotal()) == totals
    assert_bits(host(view), want[-1], "the last output after the refused calls")
    net.BackpropXent(labels)  # the last valid forward still stands
    net.PropagateFrames(corpus, frames)
    # (the parameters moved: only the Splice's gather is the same)
    assert_bits(host(net.Output(0)), want[0], "the next valid call")


def test_rows_reaching_2_31_are_refused_and_wide_contexts_clamp(kc):
    """A context of +-10^6 frames: 1100 examples would be 2^31 window rows
    (never stored, refused all the same); two examples are served, every
    spliced frame outside its utterance clamped to the utterance's ends."""
    net = kc.Nnet("SpliceComponent input-dim=4 context=-1000000:0:1000000 const-component-dim=0")
    lengths = (3, 9)
    utts = utterances(lengths, 4, 1800)
    stacked = np.concatenate(utts)
    corpus = kc.Corpus(dev(stacked), list(lengths))
    net.PropagateFrames(corpus, [1, 7])
    want = np.stack([np.concatenate([stacked[0], stacked[1], stacked[2]]),
                     np.concatenate([stacked[3], stacked[7], stacked[11]])])
    assert_bits(host(net.Output()), want, "clamped wide context")
    with pytest.raises(kc.KcnnError, match="2\\^31 rows"):
        net.PropagateFrames(corpus, [3] * 1100)
    with pytest.raises(kc.KcnnError, match="2\\^31 rows or elements"):
        net.PropagateFrames(corpus, [3] * 1073)
    assert_bits(host(net.Output()), want, "the last output after the refused calls")


# ---- train_epoch ----------------------------------------------------------------------------
def test_train_epoch_is_the_hand_written_loop(kc):
    lengths = (20, 1, 24)
    rows, mb = sum(lengths), 16
    kc.set_randn_seed(4500)
    base = kc.Nnet(CONFIGS["C"])
    utts = utterances(lengths, 6, 1900)
    corpus = kc.Corpus(dev(np.concatenate(utts)), list(lengths))
    pdfs = rng(1901).integers(0, 9, size=rows).astype(np.int32)

    def epoch(srand):
        net = base.Copy()
        seen = []
        inner = net.PropagateFrames

        def recording(c, f):
            seen.append(np.array(f, np.int32))
            inner(c, f)
        net.PropagateFrames = recording
        return net, kc.train_epoch(net, corpus, pdfs, mb, srand), seen

    net, got, seen = epoch(5)
    assert [len(f) for f in seen] == [16, 16, 13]
    order = np.random.default_rng(5).permutation(rows)
    np.testing.assert_array_equal(np.concatenate(seen), order)
    # the loop by hand, through Propagate on the windows
    twin = base.Copy()
    for at in range(0, rows, mb):
        fr = order[at:at + mb]
        twin.Propagate(dev(example_windows(utts, fr, 1, 1)))
        twin.BackpropXent([(n, int(pdfs[r]), 1.0) for n, r in enumerate(fr)])
    want = twin.ObjfTotal(reset=True)
    assert got == want and got[1] == rows, (got, want)
    assert net.ObjfTotal() == (0.0, 0.0)  # train_epoch resets the totals
    assert_same_state(kc, net, twin, "train_epoch against the loop")
    # the same srand: the same run; another: another order
    net2, got2, seen2 = epoch(5)
    assert got2 == got
    assert_same_state(kc, net2, net, "two runs with one srand")
    _, got3, seen3 = epoch(6)
    assert sorted(np.concatenate(seen3).tolist()) == list(range(rows))
    assert not np.array_equal(np.concatenate(seen3), np.concatenate(seen))
    with pytest.raises(kc.KcnnError, match="pdfs"):
        kc.train_epoch(base.Copy(), corpus, pdfs[:-1], mb, 5)
