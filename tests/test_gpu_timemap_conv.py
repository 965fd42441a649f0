"""kn_timemap_conv (nnet2/nnet-timemap-conv.hip) and kn_stream_segments
(nnet2/nnet-kernels.hip) called directly, on pitched operands with sentinels
(tests/_pitched.py).

kn_timemap_conv, out(s, g) = act(b[g] + sum_d sum_c in(s + delta d, c) w(c wc +
d wd, g)):
  * against fp64 under assert_bound(rtol=1e-5) with S = sum |terms| + |b|
    (check 1 of tests/test_gpu_compute_shared.py, the project's bar for these
    products); the fused ReLU under the same bound, ReLU being 1-Lipschitz;
  * integer data (inputs in {-2..2}, weights in {-1, 0, 1}, integer biases):
    every part of the split and every sum is exact, so the result equals numpy's
    fp32 bit for bit, with and without the ReLU, a NaN passing through it.  A
    -0 is among the inputs and the biases; the kernel's sum itself is never -0
    (the accumulators start at +0 and the lower parts of a split -0 are +0), so
    where numpy gives a zero it is +0 in both;
  * range: rows scaled by 1e6 beside rows scaled by 1e-6 and a value of 3.4e38,
    which a rounding split would turn into Inf; operands below 2^-110 get the
    elementwise bound only, the bf16x6 contract as tests/test_gpu_x6_range.py
    states it (same 2^-120, same helper: sums of ~1e-35 lie under the helper's
    absolute floor of 1e-30, so what this case pins is finite, right-sized output
    from operands whose lower parts bf16 cannot hold; the ratios are printed);
  * every refusal returns the error code and leaves the sentinels untouched.
`in` holds exactly the rows the last output row's highest tap reads, the
weights exactly the rows the strides reach, and `out` two rows more than are
computed, which keep their sentinel.

kn_stream_segments against numpy indexing, bit for bit."""
import ctypes

import numpy as np
import pytest

import _util
from _pitched import GUARD, PAD, Mat, assert_bits, stream, sync
from _util import assert_bound, rng

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 1  # hipErrorInvalidValue


@pytest.fixture(scope="module")
def KN(kc):
    lib, D = kc.lib(), kc.MatrixDim
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.kn_timemap_conv.argtypes = [P, D, P, D, P, P, D, I, I, I, I, I, I, P]
    lib.kn_timemap_conv.restype = I
    lib.kn_stream_segments.argtypes = [P, D, P, D, P, I, P]
    lib.kn_stream_segments.restype = I
    return lib


# (rows, C, group, kw, delta, layout, in stride - C, in lead, w stride - group, out stride - group):
# every rows of {1, 31, 33, 70}, C of {3, 16, 20, 40 on the Splice, 128}, group of
# {1, 5, 32, 48, 128}, kw of {1, 3, 4} and delta of {1, 2, 4}; 16-byte loads (C %
# 4 == 0, an aligned base and stride) and 4-byte ones by C, by the stride and by
# the base; a channel tail in the last chunk (C = 3, 20, 40); one and two row
# and column blocks, whole and partial.
SHAPES = [
    (1, 3, 1, 1, 1, "above", 3, 0, 3, 3),
    (31, 16, 5, 3, 2, "above", 0, 0, 0, 0),
    (33, 20, 32, 4, 4, "above", 0, 0, 0, 0),
    (70, 40, 48, 4, 1, "splice", 0, 0, 4, 4),
    (70, 128, 128, 3, 2, "above", 0, 0, 0, 0),
    (33, 128, 48, 3, 1, "above", 3, 0, 1, 1),
    (31, 16, 32, 3, 1, "above", 0, 1, 0, 0),
    (70, 40, 128, 4, 1, "splice", 3, 1, 2, 3),
    (1, 128, 128, 1, 4, "above", 4, 0, 0, 0),
    (33, 3, 5, 4, 2, "splice", 0, 0, 0, 0),
    (70, 20, 1, 3, 4, "above", 4, 0, 3, 2),
]


def name_of(s):
    return "-".join(str(v) for v in s)


def strides(layout, channels, kw):
    """(wc, wd): weight row c wc + d wd holds channel c of tap d."""
    return (1, channels) if layout == "splice" else (kw, 1)


def tap(w, d, layout, channels, kw):
    return w[d * channels:(d + 1) * channels] if layout == "splice" else w[d::kw]


def run(kc, KN, shape, x, w, b, relu, out_rows_extra=2):
    rows, channels, group, kw, delta, layout, xe, lead, we, oe = shape
    wc, wd = strides(layout, channels, kw)
    X = Mat(kc, x, extra=xe, lead=lead)
    W = Mat(kc, w, extra=we)
    B = Mat(kc, b, extra=0)
    out = Mat(kc, np.full((rows + out_rows_extra, group), PAD), extra=oe,
              guard=max(GUARD, group))
    rc = KN.kn_timemap_conv(X.ptr, X.dim, W.ptr, W.dim, B.ptr, out.ptr, out.dim, rows, kw, delta,
                            wc, wd, int(relu), stream())
    sync()
    assert rc == 0, rc
    got = out.get()
    assert (got[rows:] == PAD).all(), "rows past `rows` were written"
    assert_bits(X.get(), x, "the input")
    assert_bits(W.get(), w, "the weights")
    return got[:rows]


def fp64(shape, x, w, b):
    """(truth, S) in fp64."""
    rows, channels, group, kw, delta, layout = shape[:6]
    x64, t = x.astype(np.float64), np.tile(b.astype(np.float64), (rows, 1))
    s = np.abs(t)
    for d in range(kw):
        wd = tap(w, d, layout, channels, kw).astype(np.float64)
        assert wd.shape == (channels, group)
        a = x64[delta * d:delta * d + rows]
        assert a.shape == (rows, channels)
        t += a @ wd
        s += np.abs(a) @ np.abs(wd)
    return t, s


def operands(shape, seed):
    rows, channels, group, kw, delta = shape[:5]
    r = rng(seed)
    x = r.standard_normal((rows + delta * (kw - 1), channels)).astype(F32)
    w = (r.standard_normal((kw * channels, group)) * 0.3).astype(F32)
    b = (r.standard_normal(group) * 0.5).astype(F32)
    return x, w, b


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=name_of)
def test_against_fp64(kc, KN, shape, relu):
    x, w, b = operands(shape, 7000 + sum(shape[:5]))
    got = run(kc, KN, shape, x, w, b, relu)
    t, s = fp64(shape, x, w, b)
    if relu:
        t = np.maximum(t, 0.0)
    print(f"{name_of(shape)}: worst err / S = {(np.abs(got - t) / np.maximum(s, 1e-30)).max():.3e}")
    assert_bound(got, t, s, rtol=1e-5, what=name_of(shape))


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5], SHAPES[6], SHAPES[9]], ids=name_of)
def test_integer_data_is_numpy_bit_for_bit(kc, KN, shape, relu):
    rows, channels, group, kw, delta, layout = shape[:6]
    r = rng(7100 + rows + channels)
    x = r.integers(-2, 3, size=(rows + delta * (kw - 1), channels)).astype(F32)
    w = r.integers(-1, 2, size=(kw * channels, group)).astype(F32)
    b = r.integers(-2, 3, size=group).astype(F32)
    x[0, 0] = F32(-0.0)
    b[0] = F32(-0.0)
    nan_row = x.shape[0] // 2
    x[nan_row, channels - 1] = np.nan          # in the channel tail of the last chunk
    got = run(kc, KN, shape, x, w, b, relu)
    # numpy in fp32 on the numbers; a row that reads the NaN is NaN in every
    # column (NaN x 0 is NaN), with or without the ReLU
    hit = [nan_row - delta * d for d in range(kw) if 0 <= nan_row - delta * d < rows]
    numbers = np.where(np.isnan(x), F32(0), x)
    want = np.zeros((rows, group), F32)
    for d in range(kw):
        want = want + numbers[delta * d:delta * d + rows] @ tap(w, d, layout, channels, kw)
    want = (b[None, :] + want).astype(F32)
    assert hit and len(hit) < rows
    want[hit] = np.nan
    if relu:
        with np.errstate(invalid="ignore"):
            want = np.where(want < 0, F32(0), want).astype(F32)
        assert (want == 0).any()
    # (a NaN's payload is the matrix cores' business; every number's bits are pinned)
    assert (np.isnan(got) == np.isnan(want)).all(), "the NaNs"
    assert_bits(np.where(np.isnan(got), F32(0), got), np.where(np.isnan(want), F32(0), want),
                name_of(shape))


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4]], ids=name_of)
def test_dynamic_range(kc, KN, shape, relu):
    """Odd rows scaled by 1e6, even rows by 1e-6, and 3.4e38 in one element, the
    weights at 1e-3 so that every exact sum stays finite."""
    x, w, b = operands(shape, 7200)
    x[1::2] *= F32(1e6)
    x[0::2] *= F32(1e-6)
    x[3, 1] = F32(3.4e38)
    x[4, 2] = F32(-3.4e38)
    w = (w * F32(1e-3)).astype(F32)
    got = run(kc, KN, shape, x, w, b, relu)
    t, s = fp64(shape, x, w, b)
    assert np.isfinite(t).all() and np.abs(t).max() > 1e34
    if relu:
        t = np.maximum(t, 0.0)
    assert_bound(got, t, s, rtol=1e-5, what=name_of(shape))


@pytest.mark.parametrize("which", ["in", "w"])
def test_tiny_operands_hold_the_elementwise_bound(kc, KN, which):
    shape = SHAPES[4]
    x, w, b = operands(shape, 7300)
    tiny = F32(2.0 ** -120)
    if which == "in":
        x = (x * tiny).astype(F32)
    else:
        w = (w * tiny).astype(F32)
    b = (b * tiny).astype(F32)
    got = run(kc, KN, shape, x, w, b, False)
    t, s = fp64(shape, x, w, b)
    # the elementwise bound alone: below 2^-110 the split keeps fewer bits, and the
    # normwise error of a cancelling sum is not bounded by the contract
    print(f"tiny {which}: worst err / S = {(np.abs(got - t) / s).max():.3e}, normwise "
          f"{np.linalg.norm(got - t) / np.linalg.norm(t):.3e}")
    _util.assert_bound(got, t, s, rtol=1e-5, what=f"tiny {which}", norm_rtol=np.inf)


def test_refusals_launch_nothing(kc, KN):
    rows, channels, group, kw, delta = 5, 8, 8, 3, 2
    x = np.ones((rows + delta * (kw - 1), channels), F32)
    w = np.ones((kw * channels, group), F32)
    X, W, B = Mat(kc, x), Mat(kc, w), Mat(kc, np.ones(group, F32), extra=0)
    out = Mat(kc, np.full((rows, group), PAD))
    D = kc.MatrixDim

    def call(xp=X.ptr, xd=X.dim, wp=W.ptr, wdim=W.dim, bp=B.ptr, op=out.ptr, od=out.dim,
             rows=rows, kw=kw, delta=delta, wc=kw, wd=1):
        return KN.kn_timemap_conv(xp, xd, wp, wdim, bp, op, od, rows, kw, delta, wc, wd, 0, stream())
    refused = {
        "no input": dict(xp=None), "no weights": dict(wp=None), "no bias": dict(bp=None),
        "no output": dict(op=None), "rows 0": dict(rows=0), "kw 0": dict(kw=0),
        "delta 0": dict(delta=0), "wc 0": dict(wc=0), "wd 0": dict(wd=0),
        "the highest tap is no row of in": dict(xd=D(x.shape[0] - 1, channels, X.stride)),
        "one row more than in holds": dict(rows=rows + 1, od=D(rows + 1, group, out.stride)),
        "a dilation that leaves in": dict(delta=delta + 1),
        "the highest weight row is no row of w": dict(wdim=D(kw * channels - 1, group, W.stride)),
        "the Splice layout on fewer weight rows": dict(wc=1, wd=channels + 1),
        "out of fewer rows": dict(od=D(rows - 1, group, out.stride)),
        "out of other columns": dict(od=D(rows, group + 1, out.stride)),
        "in stride < cols": dict(xd=D(x.shape[0], channels, channels - 1)),
        "w stride < cols": dict(wdim=D(kw * channels, group, group - 1)),
        "out stride < cols": dict(od=D(rows, group, group - 1)),
    }
    for what, kw_args in refused.items():
        assert call(**kw_args) == INVALID, what
    sync()
    assert (out.get() == PAD).all()
    assert_bits(X.get(), x, "the input")
    assert call() == 0   # and the call they vary runs
    sync()
    assert (out.get() == F32(1 + kw * channels)).all()


# ---- kn_stream_segments -----------------------------------------------------------------
# (cols, arena stride - cols, arena lead, map stride - cols, map lead)
LAYOUTS = [(8, 0, 0, 0, 0), (8, 4, 0, 4, 0), (8, 3, 0, 0, 0), (8, 0, 1, 0, 0), (8, 0, 0, 0, 1),
           (5, 0, 0, 0, 0), (260, 0, 0, 0, 0), (1030, 2, 0, 2, 0)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=name_of)
def test_segments_are_numpy_indexing(kc, KN, layout):
    import torch
    cols, ae, alead, me, mlead = layout
    arena_rows = 40
    a = (np.arange(arena_rows * cols, dtype=np.int64).reshape(arena_rows, cols) + 1).astype(F32)
    a[3, 0] = F32(-0.0)
    a[20, cols - 1] = np.nan
    # {src, lo, hi, dst, rows}: T = 1 (clamped at both ends), a source below lo
    # that is negative, one clamped above, one inside its bounds, one at the
    # arena's last row; map rows 0, 1, 17 .. 19 and the last two belong to none
    segs = [(7 - 2, 7, 7, 2, 5), (-3, 0, 4, 7, 6), (12, 10, 15, 13, 4), (22, 20, 30, 20, 3),
            (36, 33, 39, 23, 9)]
    map_rows = 34
    A = Mat(kc, a, extra=ae, lead=alead)
    M = Mat(kc, np.full((map_rows, cols), PAD), extra=me, lead=mlead, guard=max(GUARD, cols))
    desc = torch.from_numpy(np.asarray(segs, np.int32).ravel()).cuda()
    assert KN.kn_stream_segments(A.ptr, A.dim, M.ptr, M.dim, desc.data_ptr(), len(segs),
                                 stream()) == 0
    sync()
    want = np.full((map_rows, cols), PAD, F32)
    for src, lo, hi, dst, rows in segs:
        want[dst:dst + rows] = a[np.clip(src + np.arange(rows), lo, hi)]
    assert (want[[0, 1, 17, 18, 19, 32, 33]] == PAD).all() and (want[2:7] == a[7]).all()
    assert_bits(M.get(), want, name_of(layout))
    assert_bits(A.get(), a, "the arena")


def test_segments_refusals(kc, KN):
    import torch
    a = np.ones((6, 8), F32)
    A, M = Mat(kc, a), Mat(kc, np.full((4, 8), PAD))
    desc = torch.from_numpy(np.asarray([0, 0, 5, 0, 4], np.int32)).cuda()
    D = kc.MatrixDim

    def call(ap=A.ptr, ad=A.dim, mp=M.ptr, md=M.dim, dp=desc.data_ptr(), num=1):
        return KN.kn_stream_segments(ap, ad, mp, md, dp, num, stream())
    for what, args in {"no arena": dict(ap=None), "no map": dict(mp=None),
                       "no descriptors": dict(dp=None), "no segments": dict(num=0),
                       "other columns": dict(md=D(4, 7, M.stride)),
                       "arena stride < cols": dict(ad=D(6, 8, 7)),
                       "map stride < cols": dict(md=D(4, 8, 7)),
                       "no map rows": dict(md=D(0, 8, M.stride))}.items():
        assert call(**args) == INVALID, what
    sync()
    assert (M.get() == PAD).all()
    assert call() == 0
    sync()
    assert (M.get() == 1).all()
