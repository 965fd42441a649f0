"""kn_timemap_gather and kn_timemap_epilogue (nnet2/nnet-timemap-kernels.hip)
called directly, bit for bit against a numpy restatement of their contract in
nnet-kernels.h, on pitched operands with sentinels (tests/_pitched.py).

The cases are tests/nnet2_kernel_cases.py's; tests/test_nnet2_routes.py pins the
kernel, grid and LDS each one launches.  Both kernels copy, compare and select:
every result is one of the input's bit patterns, -1e20f or 0.
"""
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


def unique_values(rows, cols):
    """Every element another integer (below 2^24: exact), so a copy from a wrong
    place shows; a -0.0 and a NaN among them."""
    x = (np.arange(rows * cols, dtype=np.int64).reshape(rows, cols) + 1).astype(F32)
    assert rows * cols < 2 ** 24
    x[0, 0] = F32(-0.0)
    x[rows // 2, cols // 2] = np.nan
    return x


@pytest.mark.parametrize("case", T.select("kn_timemap_gather"), ids=T.name_of)
def test_gather(kc, KN, case):
    """out(r, k + c positions) = map(r + u ext + dilation k, c)."""
    import torch
    (map_rows, channels, map_stride, map_lead), (rows, out_cols, out_stride, out_lead) = case["ops"]
    utts, n, dil, ext = case["utts"], case["positions"], case["dilation"], case["ext"]
    m = unique_values(map_rows, channels)
    M = Mat(kc, m, stride=map_stride, lead=map_lead)
    # the guard: as long as the longest run a block writes (a tile of a row)
    O = Mat(kc, np.full((rows, out_cols), np.nan), stride=out_stride, lead=out_lead,
            guard=max(GUARD, out_cols))
    starts = np.concatenate([[0], np.cumsum(utts)]).astype(np.int32)
    sd = torch.from_numpy(starts).cuda()
    assert KN.kn_timemap_gather(M.ptr, M.dim, O.ptr, O.dim, sd.data_ptr(), len(utts), ext, n, dil,
                                stream()) == 0
    sync()
    u = np.repeat(np.arange(len(utts)), utts)
    src = np.arange(rows) + u * ext
    taps = src[:, None] + dil * np.arange(n)[None, :]          # [r, k]
    assert taps.max() == map_rows - 1                          # the map's last row is read
    want = m[taps].transpose(0, 2, 1).reshape(rows, channels * n)   # [r, c, k] -> k + c n
    assert_bits(O.get(), want, case["name"])
    assert_bits(M.get(), m, "the map")
    assert (sd.cpu().numpy() == starts).all()


def fold(x, rows, cols, pw, pc, delta):
    """The reference's pool: start -1e20f, replace when v < x, over c < pc
    (outer), w < pw (inner) of in(r + delta w, oc pc + c)."""
    v = np.full((rows, cols), F32(-1e20), F32)
    with np.errstate(invalid="ignore"):
        for c in range(pc):
            for w in range(pw):
                t = x[delta * w:delta * w + rows, c::pc]
                assert t.shape == v.shape
                v = np.where(v < t, t, v)
    return v


def floor0(v):
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, F32(0), v).astype(F32)    # x < 0 -> 0: NaN and -0.0 stay


def epilogue_input(case):
    rows, cols, pw, pc, delta = (case[k] for k in ("rows", "cols", "pw", "pc", "delta"))
    in_rows, in_cols = case["ops"][0][:2]
    r = rng(rows * 131 + cols + pw + 7 * pc)
    # quarter steps in [-2, 2]: ties within a window, both signs
    x = (r.integers(-8, 9, size=(in_rows, in_cols)) * 0.25).astype(F32)
    if case["data"] == "special":
        assert cols == 8 and in_rows >= 5
        col = lambda oc: slice(oc * pc, (oc + 1) * pc)          # noqa: E731
        x[:, col(0)] = -np.inf                     # folds to -1e20f
        x[:, col(1)] = F32(-3e20)                  # below the start: -1e20f
        x[:, col(2)] = np.nan                      # an all-NaN window: -1e20f
        x[2, col(3)] = np.nan                      # a NaN among numbers never replaces
        x[::2, col(4)] = np.nan
        x[:, col(5)] = F32(-0.0)                   # -0.0 and -1: the maximum is -0.0
        x[1::2, col(5)] = F32(-1.0)
        x[3, col(6)] = np.inf
    return x


@pytest.mark.parametrize("case", T.select("kn_timemap_epilogue"), ids=T.name_of)
def test_epilogue(kc, KN, case):
    rows, cols, pw, pc, delta = (case[k] for k in ("rows", "cols", "pw", "pc", "delta"))
    in_op, p_op, r_op = case["ops"]
    x = epilogue_input(case)
    X = Mat(kc, x, stride=in_op[2], lead=in_op[3])

    def out(op):  # rows past `rows` hold the sentinel and keep it
        return Mat(kc, np.full(op[:2], PAD), stride=op[2], lead=op[3], guard=max(GUARD, op[1]))
    Pm = out(p_op) if case["pool"] else None
    Rm = out(r_op) if case["relu"] else None
    null = kc.MatrixDim(0, 0, 0)
    assert KN.kn_timemap_epilogue(X.ptr, X.dim, Pm.ptr if Pm else None, Pm.dim if Pm else null,
                                  Rm.ptr if Rm else None, Rm.dim if Rm else null, rows, pw, pc,
                                  delta, stream()) == 0
    sync()
    level = fold(x, rows, cols, pw, pc, delta) if case["pool"] else x[:rows]
    if case["pool"]:
        want = np.full(p_op[:2], PAD, F32)
        want[:rows] = level
        assert_bits(Pm.get(), want, case["name"] + ": pooled")
    if case["relu"]:
        assert_bits(Rm.get(), floor0(level), case["name"] + ": relu")
    assert_bits(X.get(), x, "the input")
    if case["data"] == "special":
        if case["pool"]:
            assert (level[:, :3] == F32(-1e20)).all()           # -inf, -3e20, all NaN
            assert not np.isnan(level).any()                    # a NaN never replaces
            assert (level[:, 3] != F32(-1e20)).all()
            assert np.signbit(level[:, 5]).all() and (level[:, 5] == 0).all()
            assert np.isinf(level[:, 6]).any()
        else:
            got = Rm.get()
            assert np.isnan(got[:, 2]).all() and np.isnan(got[2, 3])   # NaN passes the ReLU
            assert np.signbit(got[::2, 5]).all()                       # and so does -0.0
            assert (got[:, 0] == 0).all() and not np.signbit(got[:, 0]).any()
