"""The f16x3 GEMM's 256 x 256 tile (cu-gemm-f16x3.hip, gemm_f16x3_fast_kernel
with BN_WIDE), forced by the "gemm" selector's value 3.  Every case checks
through kcnn_gemm_tile_counts that the wide kernel ran (a silent fallback to
the narrow tile fails), against float64 with test_gpu_gemm.py's bound, and
where neither tile can split K (K < 2048) bitwise against the narrow tile
(value 4): both hold the same 32 x 32 accumulator blocks, summed in the same
order."""
import numpy as np
import pytest

from _util import dev, host, randn, rng
from test_gpu_gemm import RTOL, _bound, _mats

pytestmark = pytest.mark.gpu

WIDE, NARROW = 3, 4


def _run(kc, mode, fn, want_wide=True):
    """fn() under gemm = mode; asserts which tile its f16x3 launches took."""
    old = kc.get_kernel_family("gemm")
    kc.set_gemm_mode(mode)
    try:
        kc.gemm_tile_counts(reset=True)
        out = fn()
        narrow, wide = kc.gemm_tile_counts()
    finally:
        kc.set_gemm_mode(old)
    if want_wide:
        assert wide >= 1 and narrow == 0, (narrow, wide)
    else:
        assert narrow >= 1 and wide == 0, (narrow, wide)
    return out


def _check(torch, kc, m, n, k, ta, tb, alpha=1.0, beta=0.0, seed=1, pitch=0, mode=WIDE,
           want_wide=True):
    a, b, c0 = _mats(torch, m, n, k, ta, tb, seed, pitch=pitch)
    c = c0.clone()
    _run(kc, mode, lambda: kc.gemm(a, b, c, ta, tb, alpha, beta), want_wide)
    torch.cuda.synchronize()
    _bound(torch, a, b, c0, c, ta, tb, alpha, beta)
    return c


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("shape", [(256, 256, 32), (256, 256, 64), (256, 256, 96),
                                   (256, 256, 128), (300, 260, 77), (512, 768, 160)])
def test_wide_loop_tails_and_edges(kc, ta, tb, shape):
    """K of 1 to 4 steps (every entry and exit of the step loop), a shape
    ragged in M, N and K, and one of several whole tiles; all four transpose
    pairs, 16-B aligned pitches."""
    import torch
    m, n, k = shape
    _check(torch, kc, m, n, k, ta, tb, pitch=4)


@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, False), (True, True)])
def test_wide_alpha_beta_pitched(kc, ta, tb):
    import torch
    _check(torch, kc, 300, 260, 77, ta, tb, alpha=0.37, beta=1.0, pitch=12)
    _check(torch, kc, 512, 768, 160, ta, tb, alpha=-2.0, beta=0.5, pitch=4)


def test_unaligned_pitch_takes_the_narrow_tile(kc):
    """kcnn_gemm_f16x3 given a row-contiguous B whose pitch is no multiple of
    4 (AddMatMat would copy it to a padded pitch first): the one-dword loader
    has no wide kernel, so value 3 launches the narrow tile."""
    import ctypes
    import torch
    m, n, k = 300, 260, 77
    a, b, c0 = _mats(torch, m, n, k, False, False, 3, pitch=3)
    c = c0.clone()
    L = kc.lib()
    L.kl_gemm_f16x3_full_workspace_bytes.restype = ctypes.c_size_t
    wsb = int(L.kl_gemm_f16x3_full_workspace_bytes(m, n, k))
    ws = torch.empty(wsb // 4 + 4, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = L.kl_gemm_f16x3(0, 0, m, n, k, ctypes.c_float(1.0), ctypes.c_void_p(a.data_ptr()),
                             a.stride(0), ctypes.c_void_p(b.data_ptr()), b.stride(0),
                             ctypes.c_float(0.5), ctypes.c_void_p(c.data_ptr()), c.stride(0),
                             ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(wsb), stream)
        assert rc == 0, rc
    _run(kc, WIDE, call, want_wide=False)
    torch.cuda.synchronize()
    _bound(torch, a, b, c0, c, False, False, 1.0, 0.5)


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("shape", [(300, 260, 77), (512, 512, 1024)])
def test_wide_bitwise_equals_narrow(kc, ta, tb, shape):
    import torch
    m, n, k = shape
    for alpha, beta in ((1.0, 0.0), (0.5, 1.0)):
        cw = _check(torch, kc, m, n, k, ta, tb, alpha, beta, seed=4)
        cn = _check(torch, kc, m, n, k, ta, tb, alpha, beta, seed=4, mode=NARROW,
                    want_wide=False)
        assert torch.equal(cw, cn)


def test_wide_fc_component_bitwise_equals_narrow(kc):
    """A FullyConnectedComponent of 512 -> 512 on 512 frames: Propagate, the
    input derivative, and W, b and prev_grad after the momentum update fused
    into the weight-gradient GEMM's store."""
    I = Od = N = 512
    line = (f"FullyConnectedComponent input-dim={I} output-dim={Od} learning-rate=0.02 "
            f"param-stddev=0.01 bias-stddev=1 weight-decay=0.0002 momentum=0.9")
    r = rng(13)
    params = [randn(r, (Od, I), 0.05), randn(r, (Od,), 0.5), randn(r, (Od, I), 0.01)]
    x, dy = dev(randn(r, (N, I))), dev(randn(r, (N, Od), 0.1))

    def step():
        comp = kc.Component.NewFromString(line)
        for which, v in enumerate(params):
            comp.SetParam(which, dev(v))
        y = comp.Propagate(x)
        dx = comp.Backprop(x, None, dy, update=True)
        return [host(y), host(dx)] + [host(comp.GetParam(w)) for w in range(3)]
    wide = _run(kc, WIDE, step)
    narrow = _run(kc, NARROW, step, want_wide=False)
    for what, w, nr in zip(["Propagate", "dX", "W", "b", "prev_grad"], wide, narrow):
        assert np.array_equal(w, nr), what


def _forced_plan(kc, ta, tb, m, n, k, **kw):
    """The call's plan under gemm = 3 (what _run(kc, WIDE, ...) launches)."""
    old = kc.get_kernel_family("gemm")
    kc.set_gemm_mode(WIDE)
    try:
        return kc.gemm_plan(ta, tb, m, n, k, **kw)
    finally:
        kc.set_gemm_mode(old)


# (shape, split): the wide tile's plan splits K in the first two (plain split
# grid) and in the last (256 whole tiles in front of 64 split ones); the third
# is the many-tile shape of test_gemm_nonfinite_pattern, whose 184 wide tiles
# take one split
SPLIT_SHAPES = [((256, 256, 4500), True), ((512, 256, 9024), True),
                ((1024, 11616, 2048), False), ((1024, 20480, 2048), True)]


@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, False)])
@pytest.mark.parametrize("shape,split", SPLIT_SHAPES)
def test_wide_split_k(kc, ta, tb, shape, split):
    """K split over workgroups on the wide tile: the plan under the forced
    selector really splits (a silent drop to one split fails), the bound,
    run-to-run identical bits; a second shape has rows and columns past the
    last whole tile."""
    import torch
    m, n, k = shape
    tile, ksplit, nwhole = _forced_plan(kc, ta, tb, m, n, k)
    assert tile == 256 and (ksplit > 1) == split, (tile, ksplit, nwhole)
    if n == 20480:
        assert nwhole == 256, nwhole      # the whole-plus-split grid
    c1 = _check(torch, kc, m, n, k, ta, tb, beta=1.0, seed=6)
    c2 = _check(torch, kc, m, n, k, ta, tb, beta=1.0, seed=6)
    assert torch.equal(c1, c2)
    if m <= 512:
        lda = (m + 44 if ta else k) + 4
        ldb = (k if tb else n + 4) + 4
        assert _forced_plan(kc, ta, tb, m + 44, n + 4, k, lda=lda, ldb=ldb)[1] > 1
        _check(torch, kc, m + 44, n + 4, k, ta, tb, beta=1.0, seed=6, pitch=4)


def _nonfinite(torch, kc, m, n, k, ta, tb, extra_cols=()):
    """Inf / NaN rows and columns as test_gemm_nonfinite_pattern plants them
    (and a row in rows 128-255 of a tile, and extra_cols): sgemm's IEEE
    pattern exactly, the finite elements within the bound; returns C."""
    a, b, c0 = _mats(torch, m, n, k, ta, tb, seed=5)
    A = a.t() if ta else a
    B = b.t() if tb else b
    A[4, 10] = float("inf")
    A[9, 11] = float("-inf")
    A[20, 0] = float("nan")
    A[30, 12] = float("inf"); A[30, 13] = float("-inf")
    A[200, 5] = float("inf")            # rows 128-255 of the tile as well
    B[12, 7] = float("inf")
    B[:, 100] = 0.0; B[50, 100] = float("-inf")
    B[0, 60] = 0.0
    B[10, 3] = 0.0
    for j in extra_cols:
        B[33, j] = float("inf")
    c = c0.clone()
    beta = 0.5
    _run(kc, WIDE, lambda: kc.gemm(a, b, c, ta, tb, 1.0, beta))
    torch.cuda.synchronize()
    t = A.double() @ B.double() + beta * c0.double()
    fin = torch.isfinite(t)
    assert torch.equal(torch.isnan(c), torch.isnan(t))
    assert torch.equal(torch.isposinf(c), torch.isposinf(t))
    assert torch.equal(torch.isneginf(c), torch.isneginf(t))
    s = A.double().abs().nan_to_num(posinf=0) @ B.double().abs().nan_to_num(posinf=0) + \
        beta * c0.double().abs()
    err = (c.double() - t).abs()[fin]
    assert float((err / s[fin].clamp_min(1e-300)).max()) <= RTOL
    return c


@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, False)])
def test_wide_whole_plus_split_grid_nonfinite(kc, ta, tb):
    """(1024, 20480, 2048) is 4 x 80 wide tiles: the first 256 of the order
    (columns below 16384) run whole, the other 64 in 2 splits, so the reduce
    and the fix-up tell the two parts apart by the wide tile's width
    (in_split_tile).  Inf / NaN rows cross both parts and Inf columns sit in
    each (100 and 7 whole, 20000 split); identical bits over two calls."""
    import torch
    m, n, k = 1024, 20480, 2048
    assert _forced_plan(kc, ta, tb, m, n, k) == (256, 2, 256)
    c1 = _nonfinite(torch, kc, m, n, k, ta, tb, extra_cols=(20000,))
    c2 = _nonfinite(torch, kc, m, n, k, ta, tb, extra_cols=(20000,))
    assert torch.equal(torch.nan_to_num(c1), torch.nan_to_num(c2))
    assert torch.equal(torch.isnan(c1), torch.isnan(c2))


@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, False)])
@pytest.mark.parametrize("shape", [(260, 140, 300), (300, 260, 4500)])
def test_wide_nonfinite_pattern(kc, ta, tb, shape):
    """Inf / NaN rows and columns: sgemm's IEEE pattern, exactly (as
    test_gpu_gemm.py test_gemm_nonfinite_pattern); the second shape splits K."""
    import torch
    m, n, k = shape
    assert (_forced_plan(kc, ta, tb, m, n, k)[1] > 1) == (k == 4500)
    _nonfinite(torch, kc, m, n, k, ta, tb)


@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, False)])
@pytest.mark.parametrize("shape,rows", [((512, 512, 1024), (5, 300)),      # rows 0-127 of a tile
                                        ((512, 512, 1024), (200, 450)),    # rows 128-255
                                        ((300, 260, 1024), (200, 290))])   # per-register epilogue
@pytest.mark.parametrize("spread", [24, 28, 32])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_wide_spread_groups(kc, ta, tb, shape, rows, spread, beta):
    """Spread groups as test_gemm_f16x3_intra_group_range builds them: rows of
    op(A) of N(0,1) * 2^-spread but for one element whose partners are 0, so
    every element of those rows is rejected at the store and recomputed.  The
    rows sit in either half of a wave's 128 (word 0 of the rejection mask is
    the wave's rows 0-63, word 1 its rows 64-127: rows 5 and 300 fall in word
    0, 200 and 450 in word 1, the ragged shape's 200 in word 1 and 290 in word
    0), in whole tiles (the staged epilogue) and in a ragged shape (the
    per-register one); a spread column of op(B) crosses every wave row."""
    import torch
    m, n, k = shape
    a, b, c0 = _mats(torch, m, n, k, ta, tb, seed=31)
    A = a.t() if ta else a
    B = b.t() if tb else b
    g = torch.Generator(device="cuda")
    g.manual_seed(32 + spread)
    k0, k1 = k // 3, k // 3 + 1
    for i0 in rows:
        A[i0] = torch.randn(k, generator=g, device="cuda") * 2.0 ** -spread
        A[i0, k0] = 1.0
    B[k0, :] = 0.0
    j0 = n - 3
    B[:, j0] = torch.randn(k, generator=g, device="cuda") * (0.01 * 2.0 ** -spread)
    B[k1, j0] = -0.01
    B[k0, j0] = 0.0
    A[:, k1] = 0.0
    B[:, 1] = 0.0    # an all-zero column: exactly 0, not checked
    c = c0.clone()
    _run(kc, WIDE, lambda: kc.gemm(a, b, c, ta, tb, 1.0, beta))
    torch.cuda.synchronize()
    _bound(torch, a, b, c0, c, ta, tb, 1.0, beta)
    assert torch.equal(c[:, 1], c0[:, 1] * beta)
