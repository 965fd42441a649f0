"""The generic CuMatrix / CuVector kernels (kaldi-lite/cu-kernels-lite.hip)
through their kl_* launchers: kl_set, kl_scale, kl_add, kl_add_mat (both
transA), kl_copy_rows_from_vec, kl_sum_partials, kl_col_sum and kl_dot (both
transB), each against the same operation in numpy -- bit equality where the
operation is a single rounding or the data make the true result
representable, a stated rounding bound otherwise.

Matrices are pitched (stride = cols + 3 unless a case says otherwise); the
padding and 64 words after the last row hold a sentinel that must survive.

Not covered: kl_launch splits a matrix of more than 2^30 elements into
several launches; no small shape reaches that split.
"""
import ctypes
import math

import numpy as np
import pytest

from _pitched import GUARD, PAD, Mat, assert_bits, bits, stream, sync
from _util import rng

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
I = ctypes.c_int
F = ctypes.c_float
U = 2.0 ** -23   # two roundings of 2^-24 each


@pytest.fixture(scope="module")
def L(kc):
    lib, D = kc.lib(), kc.MatrixDim
    for name in ("kl_set", "kl_scale", "kl_add"):
        getattr(lib, name).argtypes = [P, D, F, P]
    lib.kl_add_mat.argtypes = [F, P, D, I, F, P, D, P]
    lib.kl_copy_rows_from_vec.argtypes = [P, P, D, P]
    lib.kl_sum_partials.argtypes = [P, I, I, I, F, P, D, P]
    lib.kl_col_sum_workspace_bytes.argtypes = [D]
    lib.kl_col_sum_workspace_bytes.restype = ctypes.c_size_t
    lib.kl_col_sum.argtypes = [P, D, F, F, P, P, P]
    lib.kl_dot.argtypes = [P, D, P, D, I, P, P]
    for name in ("kl_set", "kl_scale", "kl_add", "kl_add_mat", "kl_copy_rows_from_vec",
                 "kl_sum_partials", "kl_col_sum", "kl_dot"):
        getattr(lib, name).restype = I
    return lib


def ints(r, shape, lim=8):
    return r.integers(-lim, lim + 1, size=shape).astype(np.float32)


SHAPES = [(1, 1), (5, 257), (300, 70)]


@pytest.mark.parametrize("shape", SHAPES)
def test_set_scale_add_copy_rows(kc, L, shape):
    r = rng(shape[0])
    x = r.standard_normal(shape).astype(np.float32)
    a = np.float32(-1.7)
    m = Mat(kc, np.full(shape, np.nan))                 # kl_set overwrites NaN
    assert L.kl_set(m.ptr, m.dim, F(a), stream()) == 0
    sync()
    assert_bits(m.get(), np.full(shape, a), "kl_set")
    m = Mat(kc, x)
    assert L.kl_scale(m.ptr, m.dim, F(a), stream()) == 0
    sync()
    assert_bits(m.get(), x * a, "kl_scale")
    m = Mat(kc, x)
    assert L.kl_add(m.ptr, m.dim, F(a), stream()) == 0
    sync()
    assert_bits(m.get(), x + a, "kl_add")
    v = Mat(kc, r.standard_normal(shape[1]))
    m = Mat(kc, np.full(shape, np.nan))
    assert L.kl_copy_rows_from_vec(v.ptr, m.ptr, m.dim, stream()) == 0
    sync()
    assert_bits(m.get(), np.broadcast_to(v.get(), shape), "kl_copy_rows_from_vec")
    v.get()


def add_mat(kc, L, alpha, a, trans, beta, d):
    A, Dm = Mat(kc, a, extra=3), Mat(kc, d, extra=5)
    assert L.kl_add_mat(F(alpha), A.ptr, A.dim, int(trans), F(beta), Dm.ptr, Dm.dim, stream()) == 0
    sync()
    assert_bits(A.get(), a, "kl_add_mat's source")
    return Dm.get(), A


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("shape", [(7, 5), (70, 300), (257, 33)])
def test_add_mat(kc, L, shape, trans):
    r = rng(10 * shape[0] + trans)
    ashape = shape[::-1] if trans else shape
    a = r.standard_normal(ashape).astype(np.float32)
    y = r.standard_normal(shape).astype(np.float32)
    x = a.T if trans else a
    alpha = np.float32(0.37)
    # beta 0: fl(alpha x), whatever D held
    got, A = add_mat(kc, L, alpha, a, trans, 0.0, np.full(shape, np.nan))
    assert_bits(got, alpha * x, f"beta 0, trans {trans}")
    if trans:
        # a swapped index reads a[i * stride + j]: that read (where it stays
        # inside the source) must differ from the result
        n = min(shape[0], (A.rows * A.stride - shape[1]) // A.stride + 1)
        flat = A.h[:A.rows * A.stride]
        wrong = np.stack([flat[i * A.stride:i * A.stride + shape[1]] for i in range(n)])
        assert (bits(alpha * wrong) != bits(got[:n])).any()
    # beta 1: two roundings at most, however the expression is contracted
    got, _ = add_mat(kc, L, alpha, a, trans, 1.0, y)
    ax = np.float64(alpha) * x.astype(np.float64)
    err = np.abs(got.astype(np.float64) - (ax + y))
    lim = U * (np.abs(ax) + np.abs(y))
    assert (err <= lim).all(), f"beta 1, trans {trans}: worst err/bound {(err / lim).max():.3f}"
    # representable results: integers, power-of-two factors
    ai, yi = ints(r, ashape), ints(r, shape)
    xi = ai.T if trans else ai
    for al, be in ((0.25, 1.0), (-4.0, 1.0), (2.0, 0.5)):
        got, _ = add_mat(kc, L, al, ai, trans, be, yi)
        assert_bits(got, np.float32(al) * xi + np.float32(be) * yi, f"exact alpha {al} beta {be}")


COLS_SMALL = [1, 63, 64, 65, 256, 257]
COLS_LARGE = [70, 257]


def col_sum(kc, L, x, alpha, beta, v0, repeat=1):
    """kl_col_sum of a pitched x into a vector holding v0; the workspace is
    followed by guard words."""
    import torch
    M = Mat(kc, x)
    rows, cols = x.shape
    nbytes = L.kl_col_sum_workspace_bytes(M.dim)
    # the slab rule callers size the workspace by: slabs of a multiple of 8
    # rows, at least 16, and at most 256 slabs of one partial row each
    rps = max(16, -(-(-(-rows // 256)) // 8) * 8)
    assert nbytes == 4 * cols * -(-rows // rps) and nbytes <= 4 * cols * 256
    out = []
    for _ in range(repeat):
        # NaN where the partials go; the guard is four partial rows longer,
        # so that a final pass that takes a slab too many adds the sentinel
        ws = torch.full((nbytes // 4 + GUARD + 4 * cols,), float("nan"), dtype=torch.float32,
                        device="cuda")
        ws[nbytes // 4:] = float(PAD)
        v = Mat(kc, v0, extra=0)
        assert L.kl_col_sum(M.ptr, M.dim, F(alpha), F(beta), v.ptr, ws.data_ptr(), stream()) == 0
        sync()
        assert (ws[nbytes // 4:].cpu().numpy() == PAD).all(), "workspace guard was written"
        out.append(v.get()[0])
    M.get()
    return out


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 448, 449, 470, 4096, 4097, 4100])
def test_col_sum(kc, L, rows):
    """448 rows: 28 slabs of 16 (the final pass's tail loop alone); 449: 29
    slabs (its 8-in-flight loop); past 4096 rows: slabs of 24 rows."""
    for cols in (COLS_SMALL if rows < 448 else COLS_LARGE):
        r = rng(rows * 1000 + cols)
        # (i) integers: every partial sum is exact, the result representable
        x = ints(r, (rows, cols))
        if x[:, 0].sum() == 0:
            x[0, 0] += 1
        s = x.astype(np.float64).sum(0)
        assert s.any()                      # a dropped or doubled row shows
        v0 = (r.integers(-32, 33, size=cols) * 0.25).astype(np.float32)
        for alpha, beta in ((1.0, 0.0), (0.25, 1.0), (2.0, 0.5)):
            start = np.full(cols, np.nan, np.float32) if beta == 0.0 else v0
            want = alpha * s + (beta * v0 if beta else 0.0)
            got, = col_sum(kc, L, x, alpha, beta, start)
            assert_bits(got, want.astype(np.float32), f"{rows} x {cols} alpha {alpha} beta {beta}")
        # (ii) N(0,1): SURVEY 8(d)'s bar, and the same bits on a second call
        x = r.standard_normal((rows, cols)).astype(np.float32)
        x64 = x.astype(np.float64)
        a, b = col_sum(kc, L, x, 1.0, 0.0, np.full(cols, np.nan, np.float32), repeat=2)
        assert (bits(a) == bits(b)).all(), f"{rows} x {cols}: two calls differ"
        err, lim = np.abs(a - x64.sum(0)), 1e-5 * np.abs(x64).sum(0)
        assert (err <= lim).all(), f"{rows} x {cols}: worst err/bound {(err / lim).max():.3f}"


@pytest.mark.parametrize("m,n", [(5, 7), (33, 130)])
@pytest.mark.parametrize("S", [1, 2, 4, 5, 6, 9])
def test_sum_partials(kc, L, S, m, n):
    import torch
    r = rng(100 * S + m)
    parts = ints(r, (S, m, n))
    c0 = ints(r, (m, n))
    pd = torch.from_numpy(parts).cuda()
    for beta, start in ((0.0, np.full((m, n), np.nan)), (1.0, c0)):
        C = Mat(kc, start)
        assert L.kl_sum_partials(pd.data_ptr(), S, m, n, F(beta), C.ptr, C.dim, stream()) == 0
        sync()
        want = parts.sum(0) + (c0 if beta else 0)
        assert_bits(C.get(), want, f"S {S} beta {beta}")
    assert (pd.cpu().numpy() == parts).all()


def dot(kc, L, a, b, trans):
    import torch
    A, B = Mat(kc, a, extra=3), Mat(kc, b, extra=5)
    out = torch.full((1 + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    assert L.kl_dot(A.ptr, A.dim, B.ptr, B.dim, int(trans), out.data_ptr(), stream()) == 0
    sync()
    o = out.cpu().numpy()
    assert np.isnan(o[1:]).all(), "words after the result were written"
    A.get(), B.get()
    return float(o[0])


@pytest.mark.parametrize("shape,trans", [((1, 1), 0), ((5, 51), 0), ((16, 16), 0), ((1, 257), 0),
                                         ((37, 1000), 0), ((37, 50), 1)])
def test_dot(kc, L, shape, trans):
    """Element counts 1, 255, 256, 257 and 37000 (one block of 256 threads
    strides over them); transB: a 37 x 50 A with a 50 x 37 B."""
    r = rng(shape[1] + trans)
    bshape = shape[::-1] if trans else shape
    n = shape[0] * shape[1]
    for exact in (True, False):
        gen = (lambda s: ints(r, s)) if exact else (lambda s: r.standard_normal(s).astype(np.float32))
        a, b = gen(shape), gen(bshape)
        prod = (a.astype(np.float64) * (b.T if trans else b).astype(np.float64)).ravel()
        t = math.fsum(prod)
        got = dot(kc, L, a, b, trans)
        if exact:
            assert got == t, (shape, trans, got, t)
        else:
            # fp64 summation in any order, the products exact
            lim = n * 2.0 ** -52 * np.abs(prod).sum()
            assert abs(got - t) <= lim, (shape, trans, abs(got - t) / lim)
