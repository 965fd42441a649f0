"""kn_relu_prop / kn_relu_backprop, kn_splice_prop / kn_splice_backprop (the
chunked form) and kn_dvec_update (nnet2/nnet-kernels.hip) called directly, bit
for bit against a numpy restatement of their contract in nnet-kernels.h, on
pitched operands with sentinels (tests/_pitched.py).

The cases are tests/nnet2_kernel_cases.py's; tests/test_nnet2_routes.py pins the
kernel and grid each one launches.  Copies, compares and single roundings: every
comparison is of bits.  Where sums are formed (the ReLU statistics, the splice
derivative) the data or the stated order make the fp32 result unique.
"""
import ctypes

import numpy as np
import pytest

import nnet2_kernel_cases as T
from _pitched import GUARD, PAD, Mat, assert_bits, stream, sync
from _util import rng

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def KN(kc):
    return T.bind(kc)


def out_like(kc, op):
    rows, cols, stride, lead = op
    return Mat(kc, np.full((rows, cols), np.nan), stride=stride, lead=lead, guard=max(GUARD, cols))


def heaviside(o):
    with np.errstate(invalid="ignore"):
        return np.where(o > 0, F32(1), F32(0)).astype(F32)


def assert_bits_where_numbers(got, want, what):
    """Bits, except that a NaN the operation itself makes (0 * inf) is any NaN:
    its sign and payload are the multiplier's choice, not the contract's."""
    made = np.isnan(want)
    assert (np.isnan(got) == made).all(), f"{what}: NaNs differ"
    assert_bits(np.where(made, F32(0), got), np.where(made, F32(0), want), what)


def special_values(r, shape):
    """N(0, 1) with NaN, +-inf, +-0.0 sprinkled over it."""
    x = r.standard_normal(shape).astype(F32)
    flat = x.reshape(-1)
    vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], F32)
    at = r.choice(flat.size, size=min(flat.size, 10), replace=False)
    flat[at] = vals[np.arange(len(at)) % len(vals)]
    return x


@pytest.mark.parametrize("case", T.select("kn_relu_prop"), ids=T.name_of)
def test_relu_prop(kc, KN, case):
    """out = in with x < 0 -> 0; NaN and -0.0 stay."""
    op_in, op_out = case["ops"]
    x = special_values(rng(case["rows"] + case["cols"]), op_in[:2])
    X, Y = Mat(kc, x, stride=op_in[2], lead=op_in[3]), out_like(kc, op_out)
    assert KN.kn_relu_prop(X.ptr, X.dim, Y.ptr, Y.dim, stream()) == 0
    sync()
    with np.errstate(invalid="ignore"):
        want = np.where(x < 0, F32(0), x)
    assert_bits(Y.get(), want, case["name"])
    assert_bits(X.get(), x, "the input")
    got = Y.get()
    assert np.isnan(got[np.isnan(x)]).all() and np.signbit(got[(x == 0) & np.signbit(x)]).all()


@pytest.mark.parametrize("case", [c for c in T.select("kn_relu_backprop") if not c["stats"]],
                         ids=T.name_of)
def test_relu_backprop(kc, KN, case):
    """in_deriv = Heaviside(out_value) * out_deriv, a product: 0 * inf = NaN."""
    ov_op, od_op, id_op = case["ops"]
    r = rng(case["rows"] * 3 + case["cols"])
    ov, od = special_values(r, ov_op[:2]), special_values(r, od_op[:2])
    ov[0, 0], od[0, 0] = F32(-1.0), np.inf          # 0 * inf
    ov[-1, -1], od[-1, -1] = F32(2.0), -np.inf
    OV = Mat(kc, ov, stride=ov_op[2], lead=ov_op[3])
    OD = Mat(kc, od, stride=od_op[2], lead=od_op[3])
    ID = out_like(kc, id_op)
    assert KN.kn_relu_backprop(OV.ptr, OV.dim, OD.ptr, OD.dim, ID.ptr, ID.dim, None, None, None,
                               stream()) == 0
    sync()
    with np.errstate(invalid="ignore"):
        want = heaviside(ov) * od
    assert np.isnan(want[0, 0]) and want[-1, -1] == -np.inf
    assert_bits_where_numbers(ID.get(), want, case["name"])
    assert_bits(OV.get(), ov, "out_value")
    assert_bits(OD.get(), od, "out_deriv")


@pytest.mark.parametrize("case", [c for c in T.select("kn_relu_backprop") if c["stats"]],
                         ids=T.name_of)
def test_relu_backprop_stats(kc, KN, case):
    """value_sum += column sums of out_value, deriv_sum += those of
    Heaviside(out_value).  Integers in [-8, 8]: every fp32 partial sum is exact
    in any order, so the fp64 totals are compared for equality; they start
    non-zero and a second call adds the same again."""
    import torch
    ov_op, od_op, id_op = case["ops"]
    rows, cols = case["rows"], case["cols"]
    r = rng(rows + cols)
    ov = r.integers(-8, 9, size=(rows, cols)).astype(F32)
    od = r.integers(-8, 9, size=(rows, cols)).astype(F32)
    OV = Mat(kc, ov, stride=ov_op[2], lead=ov_op[3])
    OD = Mat(kc, od, stride=od_op[2], lead=od_op[3])
    ID = out_like(kc, id_op)
    v0 = r.integers(-32, 33, size=cols) * 0.25
    d0 = r.integers(-32, 33, size=cols) * 0.5
    # value_sum, a NaN guard, deriv_sum, a NaN guard
    sums = torch.full((2 * (cols + GUARD),), float("nan"), dtype=torch.float64, device="cuda")
    sums[:cols] = torch.from_numpy(v0).cuda()
    sums[cols + GUARD:2 * cols + GUARD] = torch.from_numpy(d0).cuda()
    nbytes = KN.kn_relu_stats_ws(OD.dim)
    assert nbytes == 2 * T.ceil(rows, 64) * cols * 4
    ws = torch.full((nbytes // 4 + GUARD,), float(PAD), dtype=torch.float32, device="cuda")
    assert ws.data_ptr() % 16 == 0
    want = heaviside(ov) * od
    colsum_v, colsum_h = ov.astype(np.float64).sum(0), heaviside(ov).astype(np.float64).sum(0)
    assert colsum_v.any() and colsum_h.any()
    for call in (1, 2):
        assert KN.kn_relu_backprop(OV.ptr, OV.dim, OD.ptr, OD.dim, ID.ptr, ID.dim,
                                   sums.data_ptr(), sums.data_ptr() + 8 * (cols + GUARD),
                                   ws.data_ptr(), stream()) == 0
        sync()
        assert_bits(ID.get(), want, f"{case['name']} call {call}")
        s = sums.cpu().numpy()
        assert (s[:cols] == v0 + call * colsum_v).all(), f"value_sum, call {call}"
        assert (s[cols + GUARD:2 * cols + GUARD] == d0 + call * colsum_h).all(), f"deriv_sum, call {call}"
        assert np.isnan(s[cols:cols + GUARD]).all() and np.isnan(s[2 * cols + GUARD:]).all()
        assert (ws[nbytes // 4:].cpu().numpy() == PAD).all(), "workspace guard was written"
    assert_bits(OV.get(), ov, "out_value")
    assert_bits(OD.get(), od, "out_deriv")


# ---- Splice -----------------------------------------------------------------------------
def in_row(c, slot, oi):
    """The in-chunk input row that block `slot` of output row oi reads."""
    if c["in_index"] is not None:
        return c["in_index"][slot * c["out_cs"] + oi]
    return c["out_first"] + oi + c["context"][slot] - c["in_first"]


def splice_prop_ref(c, x):
    ns, dim, cd = len(c["context"]), c["dim"], c["const_dim"]
    xin = x.reshape(c["num_chunks"], c["in_cs"], dim + cd)
    out = np.empty((c["num_chunks"], c["out_cs"], ns * dim + cd), F32)
    for oi in range(c["out_cs"]):
        for slot in range(ns):
            out[:, oi, slot * dim:(slot + 1) * dim] = xin[:, in_row(c, slot, oi), :dim]
        out[:, oi, ns * dim:] = xin[:, oi, dim:]          # the const tail: input row oi
    return out.reshape(c["num_chunks"] * c["out_cs"], -1)


def splice_backprop_ref(c, od):
    """in_deriv row ii: the sum over the slots c, in order, in fp32 from 0, of
    the out_deriv block of the output row whose slot c read it; the const part
    copied from output row ii (0 where there is none)."""
    ns, dim, cd = len(c["context"]), c["dim"], c["const_dim"]
    d = od.reshape(c["num_chunks"], c["out_cs"], ns * dim + cd)
    out = np.zeros((c["num_chunks"], c["in_cs"], dim + cd), F32)
    for ii in range(c["in_cs"]):
        acc = np.zeros((c["num_chunks"], dim), F32)
        for slot in range(ns):
            readers = [oi for oi in range(c["out_cs"]) if in_row(c, slot, oi) == ii]
            assert len(readers) <= 1
            if readers:
                acc = (acc + d[:, readers[0], slot * dim:(slot + 1) * dim]).astype(F32)
        out[:, ii, :dim] = acc
        if ii < c["out_cs"]:
            out[:, ii, dim:] = d[:, ii, ns * dim:]
    return out.reshape(c["num_chunks"] * c["in_cs"], -1)


@pytest.mark.parametrize("case", T.select("kn_splice_prop"), ids=T.name_of)
def test_splice_prop(kc, KN, case):
    in_op, out_op = case["ops"]
    x = rng(in_op[0]).standard_normal(in_op[:2]).astype(F32)
    X, Y = Mat(kc, x, stride=in_op[2], lead=in_op[3]), out_like(kc, out_op)
    assert KN.kn_splice_prop(X.ptr, X.dim, Y.ptr, Y.dim, T.splice_geom(case), stream()) == 0
    sync()
    assert_bits(Y.get(), splice_prop_ref(case, x), case["name"])
    assert_bits(X.get(), x, "the input")


@pytest.mark.parametrize("case", T.select("kn_splice_backprop"), ids=T.name_of)
def test_splice_backprop(kc, KN, case):
    od_op, id_op = case["ops"]
    od = rng(od_op[0] + 1).standard_normal(od_op[:2]).astype(F32)
    OD, ID = Mat(kc, od, stride=od_op[2], lead=od_op[3]), out_like(kc, id_op)
    assert KN.kn_splice_backprop(OD.ptr, OD.dim, ID.ptr, ID.dim, T.splice_geom(case),
                                 stream()) == 0
    sync()
    want = splice_backprop_ref(case, od)
    assert_bits(ID.get(), want, case["name"])
    assert_bits(OD.get(), od, "out_deriv")
    if case["name"].endswith("contiguous"):
        # rows read by one slot, by several, and (a contiguous 3-row output over a
        # 7-row chunk) every input row by at least one
        assert (want != 0).all()


# ---- kn_dvec_update ---------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.5, -2.0])
@pytest.mark.parametrize("case", T.select("kn_dvec_update"), ids=T.name_of)
def test_dvec_update(kc, KN, case, beta):
    """y = beta y + alpha x (x NULL: y = beta y).  Small integers and powers of
    two: every product and the sum are exact, fused or not."""
    import torch
    n = case["n"]
    r = rng(n)
    y = r.integers(-64, 65, size=n).astype(np.float64)
    x = r.integers(-64, 65, size=n) * 0.125
    alpha = 4.0
    yd = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    yd[:n] = torch.from_numpy(y).cuda()
    xd = torch.from_numpy(x).cuda()
    assert KN.kn_dvec_update(yd.data_ptr(), None if case["x_null"] else xd.data_ptr(),
                             ctypes.c_double(alpha), ctypes.c_double(beta), n, stream()) == 0
    sync()
    got = yd.cpu().numpy()
    want = beta * y + (0.0 if case["x_null"] else alpha * x)
    assert (got[:n] == want).all() and np.isnan(got[n:]).all()
    assert (np.signbit(got[:n]) == np.signbit(want)).all()
    assert (xd.cpu().numpy() == x).all()
