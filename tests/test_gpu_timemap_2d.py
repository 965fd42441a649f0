"""kn_timemap_conv2d, kn_timemap_pool2d and kn_timemap_gather2d
(nnet2/nnet-timemap-2d.hip) called directly, on pitched operands with sentinels
(tests/_pitched.py), the way tests/test_gpu_timemap_conv.py calls the 1-D
convolution.  A map row holds H C floats, element (h, c) at column h + c H.

kn_timemap_conv2d, out(s, oh + g OH) = act(b[g] + sum_{d, c, i} in(s + delta d,
oh + i + c H) w(i + d kh + c kh kw, g)):
  * against fp64 under assert_bound(rtol=1e-5) with S = sum |terms| + |b|, the
    project's bar for these products; the fused ReLU under the same bound, ReLU
    being 1-Lipschitz;
  * integer data (inputs in {-2..2}, weights in {-1, 0, 1}, integer biases):
    every part of the split and every sum is exact, so the result equals
    numpy's fp32 bit for bit, with and without the ReLU.  A NaN among the
    inputs makes every output whose filter window holds it NaN in every column
    (NaN x 0 is NaN) and nothing else; a -0 is among the inputs and the biases
    (the kernel's sum is never -0, so where numpy gives a zero both give +0);
  * range: rows scaled by 1e6 beside rows scaled by 1e-6 and a value of 3.4e38,
    as in the 1-D test;
  * every refusal returns the error code and leaves the sentinels untouched;
  * `in` holds exactly the rows the last output row's highest tap reads, `w`
    exactly kw C kh rows, and `out` two rows more than are computed, which keep
    their sentinel.
The shapes: an M tile (32 (row, height) pairs) that crosses time steps (OH = 5,
6, 33), one row (OH = 1: kh = H), a partial last M tile and a partial last N
tile (G = 1, 5, 48), a K tail in the last 16-wide step (kh C = 3, 9, 24), one to
24 K steps (so one, two, three and all four waves at work), aligned and
unaligned bases and strides.

kn_timemap_pool2d against a numpy restatement of the reference's fold (start
-1e20f, replace when v < x, over c (outer), w, h (inner)) and kn_timemap_gather2d
against numpy indexing, bit for bit."""
import ctypes

import numpy as np
import pytest

from _pitched import GUARD, PAD, Mat, assert_bits, stream, sync
from _util import assert_bound, rng

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 1  # hipErrorInvalidValue


@pytest.fixture(scope="module")
def KN(kc):
    lib, D = kc.lib(), kc.MatrixDim
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.kn_timemap_conv2d.argtypes = [P, D, P, D, P, P, D, I, I, I, I, I, I, I, P]
    lib.kn_timemap_conv2d.restype = I
    lib.kn_timemap_pool2d.argtypes = [P, D, P, D, P, D, I, I, I, I, I, I, P]
    lib.kn_timemap_pool2d.restype = I
    lib.kn_timemap_gather2d.argtypes = [P, D, P, D, P, I, I, I, I, I, P]
    lib.kn_timemap_gather2d.restype = I
    return lib


# (rows, H, kh, C, kw, delta, G, in stride - H C, in lead, w stride - G, out stride - OH G)
SHAPES = [
    (1, 5, 1, 1, 1, 1, 1, 3, 0, 3, 3),        # K = 1; OH 5
    (31, 5, 1, 3, 3, 2, 5, 0, 0, 0, 0),       # OH 5: tiles cross time steps; kh C = 3
    (33, 8, 3, 3, 3, 1, 32, 0, 0, 0, 0),      # kh C = 9, K = 27: two steps, a tail
    (70, 40, 8, 1, 1, 1, 48, 0, 0, 4, 4),     # c2's filter: K = 8, OH 33, a partial N tile
    (70, 8, 8, 3, 1, 2, 48, 3, 1, 1, 1),      # kh = H: OH 1; kh C = 24; unaligned base
    (33, 40, 8, 16, 3, 2, 32, 0, 0, 0, 0),    # K = 384: 24 steps
    (31, 8, 3, 16, 1, 1, 5, 0, 1, 0, 3),      # K = 48: three steps
    (70, 5, 5, 16, 3, 1, 1, 4, 0, 0, 0),      # kh = H = 5, one filter
    (33, 40, 40, 1, 3, 1, 5, 1, 0, 2, 0),     # kh = H = 40
    (1, 8, 1, 16, 3, 2, 32, 0, 0, 0, 0),      # one row, OH 8
]


def name_of(s):
    return "-".join(str(v) for v in s)


def unfold(shape, x):
    """A[(s, oh), i + d kh + c kh kw] = x[s + delta d, oh + i + c H]."""
    rows, H, kh, C, kw, delta = shape[:6]
    OH = H - kh + 1
    a = np.empty((rows, OH, kh * kw * C), x.dtype)
    for c in range(C):
        for d in range(kw):
            for i in range(kh):
                a[:, :, i + d * kh + c * kh * kw] = \
                    x[delta * d:delta * d + rows, i + c * H:i + c * H + OH]
    return a.reshape(rows * OH, -1)


def layout(shape, t):
    """[(s, oh), g] -> [s, oh + g OH]."""
    rows, H, kh = shape[:3]
    OH, G = H - kh + 1, shape[6]
    return np.ascontiguousarray(t.reshape(rows, OH, G).transpose(0, 2, 1)).reshape(rows, G * OH)


def run(kc, KN, shape, x, w, b, relu, out_rows_extra=2):
    rows, H, kh, C, kw, delta, G, xe, lead, we, oe = shape
    OH = H - kh + 1
    X = Mat(kc, x, extra=xe, lead=lead)
    W = Mat(kc, w, extra=we)
    B = Mat(kc, b, extra=0)
    out = Mat(kc, np.full((rows + out_rows_extra, OH * G), PAD), extra=oe,
              guard=max(GUARD, OH * G))
    rc = KN.kn_timemap_conv2d(X.ptr, X.dim, W.ptr, W.dim, B.ptr, out.ptr, out.dim, rows, H, C, kh,
                              kw, delta, int(relu), stream())
    sync()
    assert rc == 0, rc
    got = out.get()
    assert (got[rows:] == PAD).all(), "rows past `rows` were written"
    assert_bits(X.get(), x, "the input")
    assert_bits(W.get(), w, "the weights")
    return got[:rows]


def fp64(shape, x, w, b):
    """(truth, S) in fp64, in the output's layout."""
    a = unfold(shape, x.astype(np.float64))
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    t = a @ w64 + b64
    s = np.abs(a) @ np.abs(w64) + np.abs(b64)
    return layout(shape, t), layout(shape, s)


def operands(shape, seed):
    rows, H, kh, C, kw, delta, G = shape[:7]
    r = rng(seed)
    x = r.standard_normal((rows + delta * (kw - 1), H * C)).astype(F32)
    w = (r.standard_normal((kw * C * kh, G)) * 0.3).astype(F32)
    b = (r.standard_normal(G) * 0.5).astype(F32)
    return x, w, b


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=name_of)
def test_against_fp64(kc, KN, shape, relu):
    x, w, b = operands(shape, 7400 + sum(shape[:7]))
    got = run(kc, KN, shape, x, w, b, relu)
    t, s = fp64(shape, x, w, b)
    if relu:
        t = np.maximum(t, 0.0)
    print(f"{name_of(shape)}: worst err / S = {(np.abs(got - t) / np.maximum(s, 1e-30)).max():.3e}")
    assert_bound(got, t, s, rtol=1e-5, what=name_of(shape))


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[4], SHAPES[6]],
                         ids=name_of)
def test_integer_data_is_numpy_bit_for_bit(kc, KN, shape, relu):
    rows, H, kh, C, kw, delta, G = shape[:7]
    r = rng(7500 + rows + H + C)
    x = r.integers(-2, 3, size=(rows + delta * (kw - 1), H * C)).astype(F32)
    w = r.integers(-1, 2, size=(kw * C * kh, G)).astype(F32)
    b = r.integers(-2, 3, size=G).astype(F32)
    x[0, 0] = F32(-0.0)
    b[0] = F32(-0.0)
    x[x.shape[0] // 2, H * C - 1] = np.nan     # the last column: in the K tail's step
    got = run(kc, KN, shape, x, w, b, relu)
    a = unfold(shape, x)
    hit = np.isnan(a).any(axis=1)
    assert hit.any() and not hit.all()
    want = (b[None, :] + (np.where(np.isnan(a), F32(0), a) @ w).astype(F32)).astype(F32)
    want[hit] = np.nan
    want = layout(shape, want)
    if relu:
        with np.errstate(invalid="ignore"):
            want = np.where(want < 0, F32(0), want).astype(F32)
        assert (want == 0).any()
    # (a NaN's payload is the matrix cores' business; every number's bits are pinned)
    assert (np.isnan(got) == np.isnan(want)).all(), "the NaNs"
    assert_bits(np.where(np.isnan(got), F32(0), got), np.where(np.isnan(want), F32(0), want),
                name_of(shape))


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5]], ids=name_of)
def test_dynamic_range(kc, KN, shape, relu):
    """Odd rows scaled by 1e6, even rows by 1e-6, and 3.4e38 in one element, the
    weights at 1e-3 so that every exact sum stays finite."""
    x, w, b = operands(shape, 7600)
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


def test_conv_refusals_launch_nothing(kc, KN):
    rows, H, kh, C, kw, delta, G = 5, 6, 3, 2, 3, 2, 8
    OH = H - kh + 1
    x = np.ones((rows + delta * (kw - 1), H * C), F32)
    w = np.ones((kw * C * kh, G), F32)
    X, W, B = Mat(kc, x), Mat(kc, w), Mat(kc, np.ones(G, F32), extra=0)
    out = Mat(kc, np.full((rows, OH * G), PAD))
    D = kc.MatrixDim

    def call(xp=X.ptr, xd=X.dim, wp=W.ptr, wdim=W.dim, bp=B.ptr, op=out.ptr, od=out.dim,
             rows=rows, H=H, C=C, kh=kh, kw=kw, delta=delta):
        return KN.kn_timemap_conv2d(xp, xd, wp, wdim, bp, op, od, rows, H, C, kh, kw, delta, 0,
                                    stream())
    refused = {
        "no input": dict(xp=None), "no weights": dict(wp=None), "no bias": dict(bp=None),
        "no output": dict(op=None), "rows 0": dict(rows=0), "kw 0": dict(kw=0),
        "delta 0": dict(delta=0), "kh 0": dict(kh=0), "H 0": dict(H=0), "C 0": dict(C=0),
        "kh > H": dict(kh=H + 1),
        "the highest tap is no row of in": dict(xd=D(x.shape[0] - 1, H * C, X.stride)),
        "one row more than in holds": dict(rows=rows + 1, od=D(rows + 1, OH * G, out.stride)),
        "a dilation that leaves in": dict(delta=delta + 1),
        "the highest weight row is no row of w": dict(wdim=D(kw * C * kh - 1, G, W.stride)),
        "in of fewer columns than H C": dict(xd=D(x.shape[0], H * C - 1, X.stride)),
        "a channel more than in holds": dict(C=C + 1),
        "out of fewer rows": dict(od=D(rows - 1, OH * G, out.stride)),
        "out of other columns": dict(od=D(rows, OH * G + 1, out.stride)),
        "out for another kernel height": dict(kh=kh - 1),
        "in stride < cols": dict(xd=D(x.shape[0], H * C, H * C - 1)),
        "w stride < cols": dict(wdim=D(kw * C * kh, G, G - 1)),
        "out stride < cols": dict(od=D(rows, OH * G, OH * G - 1)),
    }
    for what, kw_args in refused.items():
        assert call(**kw_args) == INVALID, what
    sync()
    assert (out.get() == PAD).all()
    assert_bits(X.get(), x, "the input")
    assert call() == 0   # and the call they vary runs
    sync()
    assert (out.get() == F32(1 + kw * C * kh)).all()


# ---- kn_timemap_pool2d ------------------------------------------------------------------
def special_map(rows, cols, seed):
    """Numbers with NaN, +-0, +-inf and the fold's start value among them."""
    r = rng(seed)
    x = r.standard_normal((rows, cols)).astype(F32)
    x[r.random((rows, cols)) < 0.3] -= F32(2.0)  # (windows that are all negative)
    flat = x.reshape(-1)
    at = r.choice(flat.size, size=min(flat.size, 48), replace=False)
    flat[at] = np.resize(np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, -1e20, -2e20, -0.0, 0.0],
                                  F32), len(at))
    return x


def fold2d(x, rows, H, ph, pw, pc, delta):
    """The reference's Maxpool fold (start -1e20f, replace when v < x) over c <
    pc (outer), w < pw, h < ph (inner) of x[s + delta w][oh ph + h + (oc pc + c)
    H], in fp32, to [rows, oh + oc H']."""
    C = x.shape[1] // H
    OH, OC = H // ph, C // pc
    x3 = x.reshape(x.shape[0], C, H)
    v = np.full((rows, OC, OH), F32(-1e20), F32)
    with np.errstate(invalid="ignore"):
        for c in range(pc):
            for w in range(pw):
                for h in range(ph):
                    cand = x3[delta * w:delta * w + rows, c::pc, h::ph][:, :OC, :OH]
                    v = np.where(v < cand, cand, v)
    return v.reshape(rows, OC * OH)


# (rows, H, C, ph, pw, pc, delta, in stride - cols, in lead, out stride - cols)
POOLS = [(7, 6, 6, 2, 1, 1, 1, 0, 0, 0), (7, 6, 6, 1, 2, 1, 2, 3, 0, 1), (9, 5, 6, 1, 1, 3, 1, 0, 1, 0),
         (9, 6, 6, 2, 2, 2, 1, 0, 0, 0), (9, 6, 6, 2, 2, 2, 2, 2, 1, 3), (300, 33, 8, 1, 1, 4, 1, 0, 0, 0),
         (5, 6, 90, 3, 3, 1, 2, 0, 0, 0)]


@pytest.mark.parametrize("relu", [False, True], ids=["pool", "pool+relu"])
@pytest.mark.parametrize("case", POOLS, ids=name_of)
def test_pool_is_the_reference_fold(kc, KN, case, relu):
    rows, H, C, ph, pw, pc, delta, xe, lead, oe = case
    x = special_map(rows + delta * (pw - 1), H * C, 7700 + sum(case))
    cols = (H // ph) * (C // pc)
    X = Mat(kc, x, extra=xe, lead=lead)
    Pm = Mat(kc, np.full((rows + 1, cols), PAD), extra=oe, guard=max(GUARD, cols))
    Rm = Mat(kc, np.full((rows + 1, cols), PAD), extra=oe, guard=max(GUARD, cols)) if relu else None
    null = kc.MatrixDim(0, 0, 0)
    assert KN.kn_timemap_pool2d(X.ptr, X.dim, Pm.ptr, Pm.dim, Rm.ptr if relu else None,
                                Rm.dim if relu else null, rows, H, ph, pw, pc, delta,
                                stream()) == 0
    sync()
    want = fold2d(x, rows, H, ph, pw, pc, delta)
    got = Pm.get()
    assert (got[rows:] == PAD).all()
    assert_bits(got[:rows], want, f"pooled {name_of(case)}")
    if relu:
        with np.errstate(invalid="ignore"):
            act = np.where(want < 0, F32(0), want).astype(F32)
        got = Rm.get()
        assert (got[rows:] == PAD).all()
        assert_bits(got[:rows], act, f"relu {name_of(case)}")
    assert_bits(X.get(), x, "the input")


def test_pool_refusals_launch_nothing(kc, KN):
    rows, H, C, ph, pw, pc, delta = 5, 6, 4, 2, 2, 2, 2
    x = np.ones((rows + delta * (pw - 1), H * C), F32)
    cols = (H // ph) * (C // pc)
    X = Mat(kc, x)
    Pm, Rm = Mat(kc, np.full((rows, cols), PAD)), Mat(kc, np.full((rows, cols), PAD))
    D = kc.MatrixDim

    def call(xp=X.ptr, xd=X.dim, pp=Pm.ptr, pd=Pm.dim, rp=Rm.ptr, rd=Rm.dim, rows=rows, H=H,
             ph=ph, pw=pw, pc=pc, delta=delta):
        return KN.kn_timemap_pool2d(xp, xd, pp, pd, rp, rd, rows, H, ph, pw, pc, delta, stream())
    for what, args in {
            "no input": dict(xp=None), "no pooled": dict(pp=None), "rows 0": dict(rows=0),
            "delta 0": dict(delta=0), "ph 0": dict(ph=0), "pw 0": dict(pw=0), "pc 0": dict(pc=0),
            "ph does not divide H": dict(ph=4), "H does not divide the columns": dict(H=5),
            "pc does not divide C": dict(pc=3),
            "the highest tap is no row of in": dict(xd=D(x.shape[0] - 1, H * C, X.stride)),
            "pooled of other columns": dict(pd=D(rows, cols + 1, Pm.stride)),
            "pooled of fewer rows": dict(pd=D(rows - 1, cols, Pm.stride)),
            "relu of other columns": dict(rd=D(rows, cols - 1, Rm.stride)),
            "relu of fewer rows": dict(rd=D(rows - 1, cols, Rm.stride)),
            "in stride < cols": dict(xd=D(x.shape[0], H * C, H * C - 1)),
            "pooled stride < cols": dict(pd=D(rows, cols, cols - 1))}.items():
        assert call(**args) == INVALID, what
    sync()
    assert (Pm.get() == PAD).all() and (Rm.get() == PAD).all()
    assert call() == 0
    sync()
    assert (Pm.get() == 1).all() and (Rm.get() == 1).all()


# ---- kn_timemap_gather2d ----------------------------------------------------------------
# (frames of the utterances, ext, H, C, n, delta, map stride - cols, map lead, out stride - cols)
GATHERS = [((1, 7, 23, 2), 5, 5, 2, 6, 1, 0, 0, 0), ((1, 7, 23, 2), 6, 3, 8, 3, 2, 3, 1, 1),
           ((4,), 4, 2, 12, 2, 2, 0, 0, 2), ((3, 1), 10, 33, 4, 11, 1, 0, 0, 0),
           ((40,), 0, 7, 3, 1, 1, 1, 0, 0), ((2, 2), 6, 2, 600, 3, 3, 0, 0, 0)]


@pytest.mark.parametrize("case", GATHERS, ids=name_of)
def test_gather_is_numpy_indexing(kc, KN, case):
    import torch
    frames, ext, H, C, n, delta, me, mlead, oe = case
    assert delta * (n - 1) <= ext
    map_rows, total = sum(frames) + ext * len(frames), sum(frames)
    m = special_map(map_rows, H * C, 7800 + sum(case[1:]))
    starts = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
    M = Mat(kc, m, extra=me, lead=mlead)
    out = Mat(kc, np.full((total, H * C * n), PAD), extra=oe, guard=max(GUARD, H * C * n))
    sd = torch.from_numpy(starts).cuda()
    assert KN.kn_timemap_gather2d(M.ptr, M.dim, out.ptr, out.dim, sd.data_ptr(), len(frames), ext,
                                  H, n, delta, stream()) == 0
    sync()
    want = np.empty((total, C, n, H), F32)
    for u, f in enumerate(frames):
        base = int(starts[u]) + u * ext
        for k in range(n):
            want[starts[u]:starts[u] + f, :, k, :] = \
                m[base + delta * k:base + delta * k + f].reshape(f, C, H)
    assert_bits(out.get(), want.reshape(total, -1), name_of(case))
    assert_bits(M.get(), m, "the map")


def test_gather_refusals_launch_nothing(kc, KN):
    import torch
    frames, ext, H, C, n, delta = (3, 2), 2, 3, 2, 3, 1
    m = np.arange((sum(frames) + 2 * ext) * H * C, dtype=np.float32).reshape(-1, H * C)
    M = Mat(kc, m)
    out = Mat(kc, np.full((sum(frames), H * C * n), PAD))
    sd = torch.from_numpy(np.asarray([0, 3, 5], np.int32)).cuda()
    D = kc.MatrixDim

    def call(mp=M.ptr, md=M.dim, op=out.ptr, od=out.dim, sp=sd.data_ptr(), num=2, ext=ext, H=H,
             n=n, delta=delta):
        return KN.kn_timemap_gather2d(mp, md, op, od, sp, num, ext, H, n, delta, stream())
    for what, args in {
            "no map": dict(mp=None), "no output": dict(op=None), "no table": dict(sp=None),
            "no utterances": dict(num=0), "ext < 0": dict(ext=-1), "H 0": dict(H=0),
            "H does not divide the columns": dict(H=4), "n 0": dict(n=0), "delta 0": dict(delta=0),
            "out of other columns": dict(od=D(5, H * C * n + 1, out.stride)),
            "the last position is no row of the map": dict(md=D(m.shape[0] - 1, H * C, M.stride)),
            "a dilation that leaves the map": dict(delta=2),
            "map stride < cols": dict(md=D(m.shape[0], H * C, H * C - 1)),
            "out stride < cols": dict(od=D(5, H * C * n, H * C * n - 1))}.items():
        assert call(**args) == INVALID, what
    sync()
    assert (out.get() == PAD).all()
    assert call() == 0   # and the call they vary runs
    sync()
    rows = [0, 1, 2, 5, 6]   # result row r of utterance u reads map rows r + u ext + k
    want = np.stack([np.stack([m[r + k].reshape(C, H) for k in range(n)], axis=1) for r in rows])
    assert_bits(out.get(), want.reshape(5, -1), "the call itself")
    assert_bits(M.get(), m, "the map")
