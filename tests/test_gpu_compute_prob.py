"""ComputeProb (nnet-compute-prob): the objective and the frame accuracy,
forward only, on the GPU.

Two kernel paths.  The stored path reads a probability matrix P and is driven
through kcnn.comp_objf_accuracy; the fused path reads the logits of a last
SoftmaxComponent and never stores P, and is driven through a one-component
network `SoftmaxComponent dim=C`.  The expected P is what Softmax.Propagate
leaves on the device for the same input (into an output laid out as the stack
lays its own out: 16-byte aligned rows, so the input alone decides the access
width and with it the order of the row sum); the expected totals are computed
from those bits in numpy float64 with the rule of CuMatrixBase::FindRowMaxId:
a row's best column is the lowest column whose value is greater than every
earlier column's, starting from -1e21.

Bars: weight and accuracy are sums of multiples of 1/8 and must be EQUAL; the
objective within 1e-6 relative (the bar of test_gpu_nnet2_loss.py); the two
paths take log of the same bits and differ in fp64 summation order alone:
1e-12 * sum |w log p|.

test_objf_accuracy_layouts calls both launchers directly on pitched operands
with sentinels at the layouts of tests/nnet2_kernel_cases.py: every access
width at every count of values a lane holds, either side of each step, with
best columns and labels in a row's last column and element-wise tail
(tests/test_nnet2_routes.py pins the kernel of each case).
"""
import functools
import math
import os

import numpy as np
import pytest

import nnet2_kernel_cases as T
from _pitched import GUARD, assert_bits, edge_columns, stream, sync
from _pitched import place as place_op
from _util import dev, host, padded, rng, with_ties

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "models", "nnet_small.bin")
F32 = np.float32
# rows x cols: the smallest that reach each kernel form
SHAPES = [(1, 10), (37, 10), (70, 65), (37, 256),    # 4 values a lane
          (37, 257), (19, 1024),                      # 16
          (19, 1025), (9, 3454), (5, 4096),           # 64
          (5, 4097)]                                  # a block per row
LAYOUTS = ["contiguous", "padded"]
FORMS = [(6, 65), (6, 1025), (5, 4097)]  # one shape per form where every form is not needed


def place(a, layout):
    return dev(a) if layout == "contiguous" else padded(a, 5)


def device_softmax(kc, x):
    """Softmax.Propagate of the device matrix x, read back."""
    import torch
    rows, cols = x.shape
    base = torch.empty((rows, (cols + 15) // 16 * 16), dtype=torch.float32, device="cuda")
    out = base[:, :cols]
    kc.Component.NewFromString(f"SoftmaxComponent dim={cols}").Propagate(x, out=out)
    return host(out).copy()


def best_columns(p):
    """FindRowMaxId on the bits of p; -1: no best column."""
    best = np.full(p.shape[0], -1)
    for r, row in enumerate(p):
        ok = row > F32(-1e21)  # a NaN is not
        if ok.any():
            best[r] = int(np.flatnonzero(row == row[ok].max())[0])
    return best


def expected_totals(p, labels):
    best = best_columns(p)
    with np.errstate(all="ignore"):
        terms = [float(F32(w)) * float(np.log(np.float64(p[r, c]))) for r, c, w in labels]
    objf = math.fsum(terms) if all(math.isfinite(t) for t in terms) else float("nan")
    weight = math.fsum(float(F32(w)) for _, _, w in labels)
    acc = math.fsum(float(F32(w)) for r, c, w in labels if c == best[r])
    scale = math.fsum(abs(t) for t in terms if math.isfinite(t))
    return (objf, weight, acc), scale


def soft_labels(r, p):
    """Every row: 1 to 3 columns that are not its best column, weights k / 8;
    every other row its best column as well.  Sorted by (row, column)."""
    best = best_columns(p)
    rows, cols = p.shape
    out = []
    for i in range(rows):
        others = [c for c in r.choice(cols, size=min(4, cols), replace=False) if c != best[i]]
        pick = set(int(c) for c in others[:int(r.integers(1, 4))])
        if i % 2 == 0:
            pick.add(int(best[i]))
        out += [(i, c, float(r.integers(1, 9)) / 8) for c in sorted(pick)]
    return out


def tie_labels(p):
    """Each row: its first maximal column at 1.0, its last at 0.5."""
    out, split = [], 0
    for i, row in enumerate(p):
        at = np.flatnonzero(row == row.max())
        out.append((i, int(at[0]), 1.0))
        if at[-1] != at[0]:
            out.append((i, int(at[-1]), 0.5))
            split += 1
    return out, split


def stored_totals(kc, p, labels, layout):
    return kc.comp_objf_accuracy(place(p, layout), labels)


@functools.lru_cache(maxsize=None)
def softmax_net(cols):
    import kcnn
    return kcnn.Nnet(f"SoftmaxComponent dim={cols}")


def fused_totals(kc, x, labels):
    net = softmax_net(x.shape[1])
    net.ProbTotal(reset=True)
    net.ComputeProb(x, labels)
    return net.ProbTotal(reset=True)


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def check(got, want, scale, what):
    print(f"{what}: got {got!r} expected {want!r}")
    assert same(got[1], want[1]), f"{what}: weight"
    assert same(got[2], want[2]), f"{what}: accuracy"
    if math.isnan(want[0]):
        assert math.isnan(got[0]), f"{what}: objective"
    else:
        assert abs(got[0] - want[0]) <= 1e-6 * abs(want[0]), f"{what}: objective"


def check_paths_agree(fused, stored, scale):
    assert same(fused[1], stored[1]) and same(fused[2], stored[2])
    if math.isnan(stored[0]):
        assert math.isnan(fused[0])
    else:
        print(f"fused - stored = {fused[0] - stored[0]!r}, bound {1e-12 * scale!r}")
        assert abs(fused[0] - stored[0]) <= 1e-12 * scale


def run_both(kc, logits, layout, make_labels):
    """Both paths on `logits` laid out as `layout`, each twice; returns the
    expectation from the device P, and the two paths' totals."""
    x = place(logits, layout)
    p = device_softmax(kc, x)
    labels = make_labels(p)
    want, scale = expected_totals(p, labels)
    fused = [fused_totals(kc, x, labels) for _ in range(2)]
    stored = [stored_totals(kc, p, labels, layout) for _ in range(2)]
    # determinism: identical bits for all three totals
    for a, b in (fused, stored):
        assert all(same(u, v) for u, v in zip(a, b)), (a, b)
    check(stored[0], want, scale, "stored")
    check(fused[0], want, scale, "fused")
    check_paths_agree(fused[0], stored[0], scale)
    return p, labels, want


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_logits(kc, shape, layout):
    r = rng(shape[0] * 10007 + shape[1])
    logits = (r.standard_normal(shape) * 3).astype(F32)
    _, _, want = run_both(kc, logits, layout, lambda p: soft_labels(r, p))
    # about half the rows are labelled with their best column: a constant
    # answer cannot pass
    assert 0 < want[2] < want[1]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tied_maxima_take_the_lowest_column(kc, shape, layout):
    logits = with_ties(rng(shape[1]), shape, levels=7)
    split = []

    def labels(p):
        lab, n = tie_labels(p)
        split.append(n)
        return lab
    p, _, want = run_both(kc, logits, layout, labels)
    rows, cols = shape
    if cols >= 257:
        assert split[0] == rows  # every row has a tied maximum
    elif shape == (70, 65):
        assert split[0] >= 60
    # the first maximal column scores, the last does not
    assert want[2] == rows and want[1] == rows + 0.5 * split[0]


@pytest.fixture(scope="module")
def KN(kc):
    return T.bind(kc)


@pytest.mark.parametrize("case", T.select("kn_objf_accuracy") + T.select("kn_softmax_objf_accuracy"),
                         ids=T.name_of)
def test_objf_accuracy_layouts(kc, KN, case):
    """The stored path on P, the fused path on the logits, in the case's layout.
    The expected P: kn_softmax_prop of the logits in that layout into a 16-byte
    aligned output (nnet-kernels.h).  Every other row is labelled with its best
    column (soft_labels), and that is one of the edge columns in turn, the last
    column first."""
    import torch
    rows, cols = case["rows"], case["cols"]
    fused = case["launcher"] == "kn_softmax_objf_accuracy"
    r = rng(rows * 10007 + cols + fused)
    logits = (r.standard_normal((rows, cols)) * 3).astype(F32)
    edges = edge_columns(cols)[::-1]
    for i in range(0, rows, 2):
        logits[i, edges[(i // 2) % len(edges)]] = F32(20.0)
    X = place_op(kc, case["ops"][0], logits)
    Pm = place_op(kc, (rows, cols) + T.layout(cols, "v4"))
    assert KN.kn_softmax_prop(X.ptr, X.dim, Pm.ptr, Pm.dim, stream()) == 0
    sync()
    p = Pm.get()
    assert best_columns(p)[0] == edges[0] == cols - 1
    labels = soft_labels(r, p)
    assert all((i, edges[(i // 2) % len(edges)]) in {lab[:2] for lab in labels}
               for i in range(0, rows, 2))
    want, scale = expected_totals(p, labels)
    assert 0 < want[2] <= want[1]
    count = np.bincount([lab[0] for lab in labels], minlength=rows)
    row_start = torch.from_numpy(np.concatenate([[0], np.cumsum(count)]).astype(np.int32)).cuda()
    lab_col = torch.from_numpy(np.array([lab[1] for lab in labels], np.int32)).cuda()
    lab_w = torch.from_numpy(np.array([lab[2] for lab in labels], F32)).cuda()
    Q = X if fused else place_op(kc, case["ops"][0], p)
    n = KN.kn_prob_ws(KN.kn_prob_blocks(Q.dim)) // 8
    got = []
    for _ in range(2):
        ws = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        tot = torch.full((3 + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        tot[:3] = 0
        launcher = KN.kn_softmax_objf_accuracy if fused else KN.kn_objf_accuracy
        assert launcher(Q.ptr, Q.dim, row_start.data_ptr(), lab_col.data_ptr(), lab_w.data_ptr(),
                        tot.data_ptr(), ws.data_ptr(), stream()) == 0
        sync()
        t = tot.cpu().numpy()
        assert np.isnan(t[3:]).all() and np.isnan(ws[n:].cpu().numpy()).all()
        got.append(tuple(float(v) for v in t[:3]))
    assert all(same(u, v) for u, v in zip(*got)), got
    check(got[0], want, scale, case["name"])
    assert_bits(Q.get(), logits if fused else p, "the input")


def special_matrix(kind, shape):
    """Random logits whose row 2 is special; its labels; the matrix and labels
    without that row."""
    rows, cols = shape
    r = rng(cols + len(kind))
    logits = (r.standard_normal(shape) * 3).astype(F32)
    marked = sorted(int(c) for c in r.choice(cols, size=3, replace=False))
    if kind == "nan":
        logits[2, marked[1]] = np.nan
    elif kind == "-inf":
        logits[2, :] = -np.inf
    else:  # the labelled columns underflow to the 1e-20 floor
        logits[2, marked] = -200.0
    return logits, [(2, c, k / 8) for c, k in zip(marked, (8, 3, 5))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["nan", "-inf", "floor"])
@pytest.mark.parametrize("shape", FORMS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_special_rows(kc, shape, kind, layout):
    logits, special = special_matrix(kind, shape)
    x = place(logits, layout)
    p = device_softmax(kc, x)
    if kind == "floor":
        assert all(p[2, c] == F32(1e-20) for _, c, _ in special)
    else:
        assert np.isnan(p[2]).all()
    keep = [i for i in range(shape[0]) if i != 2]
    others = [(i, c, w) for i, c, w in soft_labels(rng(5), p) if i != 2]
    labels = sorted(others + special)
    want, scale = expected_totals(p, labels)
    assert math.isnan(want[0]) == (kind != "floor")
    fused = fused_totals(kc, x, labels)
    stored = stored_totals(kc, p, labels, layout)
    check(stored, want, scale, "stored")
    check(fused, want, scale, "fused")
    check_paths_agree(fused, stored, scale)
    # the same matrix without the special row: what the other rows add is
    # what they added beside it
    renum = {old: new for new, old in enumerate(keep)}
    less = [(renum[i], c, w) for i, c, w in others]
    x2 = place(logits[keep], layout)
    p2 = device_softmax(kc, x2)
    assert (p2.view(np.int32) == p[keep].view(np.int32)).all()
    want2, scale2 = expected_totals(p2, less)
    sw = math.fsum(float(F32(w)) for _, _, w in special)
    for name, got, got2 in (("fused", fused, fused_totals(kc, x2, less)),
                            ("stored", stored, stored_totals(kc, p2, less, layout))):
        check(got2, want2, scale2, name + " without the special row")
        assert got[1] == got2[1] + sw and got[2] == got2[2], name
        if kind == "floor":
            add = math.fsum(float(F32(w)) * math.log(float(F32(1e-20))) for _, _, w in special)
            assert abs((got[0] - got2[0]) - add) <= 1e-12 * scale, name


FC = ("FullyConnectedComponent input-dim={i} output-dim={o} learning-rate=0.02 "
      "param-stddev={s} bias-stddev=0.5 weight-decay=0.0005 momentum=0.9")


@pytest.mark.parametrize("literal", [False, True])
def test_refused_labels_run_nothing(kc, literal):
    kc.set_randn_seed(78)
    net = kc.Nnet(FC.format(i=24, o=10, s=0.3) + "\nSoftmaxComponent dim=10")
    x = dev(rng(9).standard_normal((37, 24)).astype(F32))
    r = rng(10)
    good = [(i, int(r.integers(10)), 1.0) for i in range(37)]
    bad = {"outside": [good[:5] + [(37, 0, 1.0)], good[:5] + [(-1, 0, 1.0)],
                       good[:5] + [(5, 10, 1.0)], [(0, -1, 1.0)]],
           "not sorted": [[good[4], good[3]]],
           "repeated": [[good[3], good[3]], [(3, 1, 0.5), (3, 2, 0.25), (3, 1, 0.25)]]}
    kc.set_literal_path(literal)
    try:
        for what, cases in bad.items():
            for labels in cases:
                with pytest.raises(kc.KcnnError, match=what):
                    net.ComputeProb(x, labels)
        assert net.ProbTotal() == (0.0, 0.0, 0.0)
        with pytest.raises(kc.KcnnError):  # 23 columns for a 24-column network
            net.ComputeProb(dev(np.zeros((37, 23), F32)), good)
        assert net.ProbTotal() == (0.0, 0.0, 0.0)
        net.ComputeProb(x, good)
        objf, w, acc = net.ProbTotal()
        assert w == 37 and np.isfinite(objf) and objf < 0 and 0 <= acc <= 37
    finally:
        kc.set_literal_path(False)
    for what, labels in (("outside", [(0, 10, 1.0)]), ("repeated", [good[3], good[3]])):
        with pytest.raises(kc.KcnnError, match=what):
            kc.comp_objf_accuracy(dev(np.full((37, 10), 0.1, F32)), labels)


# ---- whole networks ---------------------------------------------------------------
def bits_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def snapshot(net):
    """Every parameter and PrevGrad (device), every NonlinearComponent statistic."""
    params, stats = [], []
    for c in net.components:
        if c.NumGradientParams() > 0:
            params += [c.GetParam(w) for w in (0, 1, 2)]
        elif c.Type() in ("RectifiedLinearComponent", "SoftmaxComponent", "NormalizeComponent"):
            vs, ds, cnt = c.NonlinearStats()
            stats.append((vs.copy(), ds.copy(), cnt))
    return params, stats


def assert_unchanged(before, after):
    for a, b in zip(before[0], after[0]):
        assert bits_equal(a, b), "a parameter changed"
    assert len(before[1]) == len(after[1])
    for (v0, d0, c0), (v1, d1, c1) in zip(before[1], after[1]):
        np.testing.assert_array_equal(v0, v1)
        np.testing.assert_array_equal(d0, d1)
        assert c0 == c1


def reseed(net):
    """The same Dropout masks for the next forward pass of every run."""
    for c in net.components:
        if c.Type() == "DropoutComponent":
            c.SetDropoutSeed(1234)


def small_net(kc):
    net = kc.Nnet.Read(FIXTURE)
    x = dev(rng(21).standard_normal((3 * 40, 8)).astype(F32))
    return net, x


def nnet_config_test_model(kc):
    scales = [float(s) for s in
              open(os.path.join(GOLDEN, "dropout_scale.config")).read().strip().split(":")]
    kc.set_randn_seed(2028)
    net = kc.Nnet(open(os.path.join(GOLDEN, "nnet.config")).read())
    net.components[-2].PerturbParams(0.05)  # the last FC starts at zero
    x = dev(rng(22).standard_normal((8 * 21, 40)).astype(F32))
    return net.Copy(scales=scales, remove_dropout=True), x


@pytest.mark.parametrize("make", [small_net, nnet_config_test_model])
def test_whole_network(kc, make):
    net, x = make(kc)
    last = net.NumComponents() - 1
    reseed(net)
    net.Propagate(x)
    p = host(net.Output()).copy()
    labels = soft_labels(rng(23), p)
    want, scale = expected_totals(p, labels)
    assert 0 < want[2] < want[1]
    before = snapshot(net)
    got = {}
    for literal in (False, True):
        kc.set_literal_path(literal)
        try:
            reseed(net)
            net.ComputeProb(x, labels)
            got[literal] = net.ProbTotal(reset=True)
            # the documented after-state: nothing to backpropagate until the
            # next Propagate; the last output is there on request
            for call in (lambda: net.BackpropXent(labels),
                         lambda: net.Backprop(dev(np.zeros_like(p))),
                         lambda: net.BackpropComponent(last, dev(np.zeros_like(p)))):
                with pytest.raises(kc.KcnnError, match="propagate first"):
                    call()
            assert (host(net.Output()).view(np.int32) == p.view(np.int32)).all()
        finally:
            kc.set_literal_path(False)
        check(got[literal], want, scale, "literal" if literal else "fused")
    check_paths_agree(got[False], got[True], scale)
    assert_unchanged(before, snapshot(net))
    assert net.ObjfTotal() == (0.0, 0.0)  # the training totals are another pair
    # the training step's objective on a copy, from the same labels
    copy = net.Copy()
    reseed(copy)
    copy.Propagate(x)
    copy.BackpropXent(labels)
    objf, weight = copy.ObjfTotal()
    assert weight == want[1] and abs(objf - got[False][0]) <= 1e-6 * abs(objf)
    assert copy.ProbTotal() == (0.0, 0.0, 0.0)
    # and after a Propagate the network trains again
    reseed(net)
    net.Propagate(x)
    net.BackpropXent(labels)
    assert net.ObjfTotal()[1] == want[1] and net.ProbTotal() == (0.0, 0.0, 0.0)


def test_totals_accumulate_and_reset(kc):
    net, x = small_net(kc)
    net = net.Copy(remove_dropout=True)
    net.Propagate(x)
    labels = soft_labels(rng(24), host(net.Output()))
    net.ComputeProb(x, labels)
    one = net.ProbTotal()
    net.ComputeProb(x, labels)
    two = net.ProbTotal(reset=True)
    assert two[1] == 2 * one[1] and two[2] == 2 * one[2]
    assert abs(two[0] - 2 * one[0]) <= 1e-12 * abs(two[0])
    assert net.ProbTotal() == (0.0, 0.0, 0.0)
    net.ComputeProb(x, [])  # no labels: the forward pass alone
    assert net.ProbTotal() == (0.0, 0.0, 0.0)
