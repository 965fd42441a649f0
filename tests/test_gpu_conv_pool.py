"""The fused conv + pool entry points at the C ABI, case by case over
tests/conv_pool_cases.py (tests/test_conv_pool_routes.py pins the kernel each
case launches): hipF_conv2d_maxpool[3d] and kcnn_conv2d_maxpool_stats against
the oracle's convolution and the header's definitions of the pooled output and
the routing mask; hipF_conv2d_backward_pooled[3d] against the oracle's Backprop
and gradient of the derivative the mask routes.

Operands are tests/_pitched.py matrices with sentinels (the masks in a byte
buffer of the same kind): what a kernel must not write is asserted after every
call.  The bar is the project's: _util.assert_bound, rtol 1e-5 elementwise on
S and normwise; everything a select defines is compared bit for bit.
"""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import conv_pool_cases as T
import conv_pool_ref as PR
import oracle as O
from _pitched import Mat, assert_bits, place, stream, sync
from _util import assert_bound, assert_same, dev, randn, rng, triple, with_ties
from test_gpu_pool_stats import PoolStatsOut, expected as stats_expected

pytestmark = pytest.mark.gpu

VP, Z = ctypes.c_void_p, ctypes.c_size_t


@pytest.fixture
def families(kc):
    old = {n: kc.get_kernel_family(n) for n in T.FAMILY_DEFAULT}

    def set_(c):
        for n, v in T.families(c).items():
            kc.set_kernel_family(n, v)
    yield set_
    for n, v in old.items():
        kc.set_kernel_family(n, v)


class MaskBuf:
    """A pitched device matrix of 1- or 2-byte mask elements with sentinels
    before the base, in the padding of every row and after the last row."""

    def __init__(self, op, elem, values=None):
        import torch
        self.rows, self.cols, self.stride, self.lead = op
        self.dt = np.uint8 if elem == 1 else np.uint16
        self.sent = self.dt(0xA5 if elem == 1 else 0xA5A5)
        self.h = np.full(self.lead + self.rows * self.stride + max(64, self.cols), self.sent,
                         self.dt)
        if values is not None:
            self.body(self.h)[:, :self.cols] = values
        self.t = torch.from_numpy(self.h.view(np.uint8).copy()).cuda()
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + elem * self.lead

    def body(self, h):
        return h[self.lead:self.lead + self.rows * self.stride].reshape(self.rows, self.stride)

    def get(self):
        g = self.t.cpu().numpy().view(self.dt)
        assert (g[:self.lead] == self.sent).all(), "the mask elements before the base were written"
        assert (self.body(g)[:, self.cols:] == self.sent).all(), "the mask's padding was written"
        assert (g[self.lead + self.rows * self.stride:] == self.sent).all(), "mask guard written"
        return self.body(g)[:, :self.cols].astype(np.uint32)


def untouched(m, what):
    """An output the call was not given (or must not write) is still NaN."""
    assert np.isnan(m.get()).all(), f"{what} was written"


def seed_of(c):
    return zlib.crc32(c["name"].encode()) & 0x7FFFFFFF


def make_data(c, g):
    """X, W, b of the case's data kind."""
    r = rng(seed_of(c))
    kind, pc = c["data"], c["win"][2]
    x = randn(r, (g.R, g.CHW))
    Wm = randn(r, (g.Kdim, g.G), 1.0 / np.sqrt(g.Kdim))
    bv = randn(r, (g.G,))
    if kind == "ties":       # the maps of every pool group identical, and ties over positions
        x = with_ties(r, x.shape)
        for j in range(g.G // pc):
            Wm[:, j * pc:(j + 1) * pc] = Wm[:, j * pc:j * pc + 1]
            bv[j * pc:(j + 1) * pc] = bv[j * pc]
    elif kind == "special":  # an Inf frame, a NaN frame, a 2^-30 pool group under a zero frame
        assert g.R >= 5 and g.G // pc > 1
        x[1, 3] = np.inf
        x[2, 5] = np.nan
        x[3] = 0.0
        bv[pc:2 * pc] = np.float32(2.0 ** -30)
    elif kind == "spread":   # test_gpu_pool_stats.py's spread frames and columns
        assert g.R > 30 and g.G // pc > 10
        bv[5 * pc:6 * pc] = np.float32(2.0 ** -30)
        bv[9 * pc:10 * pc] = np.float32(2.0 ** -19)
        x[[10, 11, g.R - 1]] = 0.0
        x[20] *= np.float32(2.0 ** -25)
    elif kind == "reject":   # test_gpu_igemm_f16.py's "filter" group range: the f16x3 check rejects
        taps = g.kh * g.kw
        Wm[:taps] = 1.0
        Wm[taps:] *= np.float32(2.0 ** -28)
        x.reshape(g.R, g.C, g.H * g.W)[:, 0] = 0.0
        bv[:] = 0.0
    else:
        assert kind == "randn"
    return x, Wm, bv


def oracle_conv(g, Wm, bv):
    oc = O.Conv(g.H, g.W, g.C, g.kh, g.kw, g.G, g.pad_h, g.pad_w)
    oc.W, oc.b = Wm.copy(), bv.copy()
    return oc


def shape_args(g):
    return g.H, g.W, g.C, g.pad_h, g.pad_w


def workspace(nbytes):
    import torch
    t = torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device="cuda")
    return t, VP(t.data_ptr()), Z(int(nbytes))


def conv2d_unfused(kc, g, X, Wd, B):
    """hipF_conv2d (concat) into a dense Y, under the families now set."""
    L = kc.lib()
    L.hipF_conv2d_workspace_bytes.restype = Z
    Y = Mat(kc, np.full((g.R, g.P * g.G), np.nan), extra=0)
    ws = workspace(L.hipF_conv2d_workspace_bytes(X.dim, g.H, g.W, g.C, g.pad_h, g.pad_w, g.kh,
                                                 g.kw, g.G))
    rc = L.hipF_conv2d(VP(X.ptr), X.dim, *shape_args(g), VP(Wd.ptr), Wd.dim, g.kh, g.kw, g.G,
                       VP(B.data_ptr()), VP(Y.ptr), Y.dim, 1, ws[1], ws[2], VP(stream()))
    sync()
    assert rc == 0
    return Y


def maxpool_unfused(kc, g, Y, win):
    ph, pw, pc = win
    Pm = Mat(kc, np.full((g.R, g.P * g.G // (ph * pw * pc)), np.nan), extra=0)
    rc = kc.lib().hipF_maxpool_prop(VP(Y.ptr), Y.dim, VP(Pm.ptr), Pm.dim, g.oh, g.ow, ph, pw, pc,
                                    0, VP(stream()))
    sync()
    assert rc == 0
    return Pm.get()


def run_forward(kc, c, g, X, Wd, B, y_stored, entry=None, lay=True):
    """One call of the case's forward entry into fresh outputs:
    (rc, Y matrix, pooled, mask, statistics or None)."""
    import torch
    L = kc.lib()
    entry = entry or c["entry"]
    ph, pw, pc = c["win"]
    ops = {n: (T.op(c, n) if lay else T.op(c, n)[:2] + (T.op(c, n)[1], 0)) for n in "ypm"}
    Y, PL = place(kc, ops["y"]), place(kc, ops["p"])
    MK = MaskBuf(ops["m"], 2 if entry == "maxpool3d" else 1)
    args = [VP(X.ptr), X.dim, *shape_args(g), VP(Wd.ptr), Wd.dim, g.kh, g.kw, g.G,
            VP(B.data_ptr()), VP(Y.ptr) if y_stored else None, Y.dim, VP(PL.ptr), PL.dim,
            VP(MK.ptr), MK.stride]
    st = keep = None
    if entry == "maxpool3d":
        rc = L.hipF_conv2d_maxpool3d(*args, ph, pw, pc, VP(stream()))
    elif entry == "maxpool":
        rc = L.hipF_conv2d_maxpool(*args, pc, VP(stream()))
    else:
        L.kcnn_conv2d_maxpool_stats_words.restype = Z
        words = L.kcnn_conv2d_maxpool_stats_words(g.R, g.H, g.W, g.C, g.kh, g.kw, g.G, pc)
        assert words > 0
        room = entry == "maxpool_stats"
        keep = [torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                for n in (3 * g.R, 3 * PL.cols, words)]
        st = PoolStatsOut(keep[0].data_ptr(), keep[1].data_ptr(),
                          keep[2].data_ptr() if room else None, words if room else 0, 0)
        rc = L.kcnn_conv2d_maxpool_stats(*args, pc, VP(stream()), ctypes.byref(st))
    sync()
    if rc != 0:
        return rc, None, None, None, None
    stats = None
    if st is not None:
        stats = (st.produced, keep[0].cpu().numpy().view(np.uint32),
                 keep[1].cpu().numpy().view(np.uint32))
    if not y_stored:
        untouched(Y, "Y (NULL in the call)")
    return rc, Y, PL.get(), MK.get(), stats


@pytest.mark.parametrize("case", T.select(T.FORWARDS), ids=T.name_of)
def test_forward(kc, families, case):
    c, g = case, T.Geom(case["shape"], case["rows"])
    families(c)
    win = c["win"]
    x, Wm, bv = make_data(c, g)
    X, Wd, B = place(kc, T.op(c, "x"), x), place(kc, T.op(c, "w"), Wm), dev(bv)
    fixes = (ctypes.c_ulonglong * 3)()
    kc.lib().kcnn_conv_fix_counts(fixes, 1)
    rc, Ym, pooled, mask, stats = run_forward(kc, c, g, X, Wd, B, True)
    assert rc == 0
    kc.lib().kcnn_conv_fix_counts(fixes, 1)
    if c["data"] == "reject":   # the fix-up kernels had tiles or elements to recompute
        assert fixes[0] == 1 and fixes[1] + fixes[2] > 0, list(fixes)
    y = Ym.get()
    rc0, _, pooled0, mask0, stats0 = run_forward(kc, c, g, X, Wd, B, False)
    assert rc0 == 0
    X.get(), Wd.get()                                   # the inputs' sentinels
    # Y NULL: the same pooled output and mask, bit for bit
    assert_same(pooled0, pooled, "pooled output, Y NULL vs Y stored")
    assert (mask0 == mask).all(), "mask, Y NULL vs Y stored"
    finite = np.isfinite(x).all(axis=1)
    if c["data"] == "special":
        # against the unfused convolution followed by hipF_maxpool_prop, NaN equal to NaN
        assert not finite.all()
        Yu = conv2d_unfused(kc, g, X, Wd, B)
        assert_same(y, Yu.get(), "Y vs the unfused convolution")
        assert_same(pooled, maxpool_unfused(kc, g, Yu, win), "pooled vs the unfused pair")
    else:
        assert_same(pooled, O.maxpool_prop(y, g.oh, g.ow, *win, pooled.shape[1]),
                    "pooled vs Maxpool_prop of the call's own Y")
    if "fwd rp" in c["tags"]:    # the two calls took different kernels: the unfused one too
        yu = conv2d_unfused(kc, g, X, Wd, B).get()
        assert_same(pooled0[finite], O.maxpool_prop(yu, g.oh, g.ow, *win, pooled.shape[1])[finite],
                    "register-pooled output vs Maxpool_prop of the unfused convolution")
    # the mask is the header's definition, from that Y and that pooled output
    nonan = ~np.isnan(y).any(axis=1)
    want = PR.mask_of(y, pooled, g.G, g.oh, g.ow, win)
    assert (mask[nonan] == want[nonan]).all(), "mask differs from the header's definition"
    # the oracle: Y at the bar, and the pooled output independently of the kernel's own Y
    oc = oracle_conv(g, Wm, bv)
    xf = x[finite]
    _, y_t, y_s = triple(lambda: oc.propagate(xf))
    assert_bound(y[finite], y_t, y_s, what=f"{c['name']} Y")
    p_t = PR.max_window(y_t, g.G, g.oh, g.ow, win).astype(np.float64)
    p_s = PR.max_window(y_s, g.G, g.oh, g.ow, win).astype(np.float64)
    err = np.abs(pooled[finite].astype(np.float64) - p_t)
    assert (err <= 1e-5 * p_s + 1e-30).all(), \
        f"pooled vs the pooled truth: worst err/S {(err / np.maximum(p_s, 1e-30)).max():.3e}"
    # the statistics entry
    which = stats if c["outs"] == "Y" else stats0
    if which is not None:
        produced, rows, cols = which
        assert produced == c["produced"]
        if produced:
            Pm = pooled0 if c["outs"] == "noY" else pooled
            row_e, col_e, nrs, ncs = stats_expected(Pm)
            if c["data"] == "spread":
                assert nrs > 0 and ncs > 0, (nrs, ncs)
            for name, got, exp, n in (("row", rows, row_e, g.R), ("col", cols, col_e, Pm.shape[1])):
                for k, part in enumerate(("max", "min", "cnt")):
                    bad = np.flatnonzero(got[k * n:(k + 1) * n] != exp[k * n:(k + 1) * n])
                    assert bad.size == 0, f"{name} {part} differs at {bad[:5]}"
    else:
        assert c["produced"] == 0


# ---- backward -------------------------------------------------------------------------------
def make_mask(kc, c, g, r, x, Wm, X, Wd):
    """The routing mask of the case's source, [R, pooled columns] of uint32."""
    win = c["win"]
    ncol, nbits = T.pooled_cols(c), win[0] * win[1] * win[2]
    if c["mask"] == "ones":
        return np.full((g.R, ncol), PR.window_bits(win), np.uint32)
    if c["mask"] == "zeros":
        return np.zeros((g.R, ncol), np.uint32)
    if c["mask"] == "random":
        return r.integers(0, 1 << nbits, size=(g.R, ncol)).astype(np.uint32)
    # the forward entry's own mask; where it declines (P past 384), the definition's
    bv = randn(r, (g.G,))
    if c["data"] == "ties":
        bv = np.repeat(bv[::win[2]], win[2])
    fwd = "maxpool" if c["entry"] == "bpool" else "maxpool3d"
    rc, _, _, mask, _ = run_forward(kc, c, g, X, Wd, dev(bv), False, entry=fwd, lay=False)
    if rc == 0:
        return mask
    assert rc == T.DECLINED
    y = oracle_conv(g, Wm, bv).propagate(x)
    return PR.mask_of(y, PR.max_window(y, g.G, g.oh, g.ow, win), g.G, g.oh, g.ow, win)


def run_backward(kc, c, g, X, Wd, src, MK, dx, gw, entry=None):
    """One call of a backward entry into fresh outputs: (rc, dX, gW, gb);
    src is dP (pooled entries) or dY."""
    import torch
    L = kc.lib()
    entry = entry or c["entry"]
    ph, pw, pc = c["win"]
    L.hipF_conv2d_backward_workspace_bytes.restype = Z
    ws = workspace(L.hipF_conv2d_backward_workspace_bytes(X.dim, *shape_args(g), g.kh, g.kw, g.G))
    DX, GW = place(kc, T.op(c, "dx")), place(kc, T.op(c, "gw"))
    gb = torch.full((g.G + 64,), float("nan"), dtype=torch.float32, device="cuda")
    tail = [VP(Wd.ptr), Wd.dim, g.kh, g.kw, g.G, VP(DX.ptr) if dx else None, DX.dim,
            VP(GW.ptr) if gw else None, GW.dim, VP(gb.data_ptr()) if gw else None, ws[1], ws[2],
            VP(stream())]
    head = [VP(X.ptr), X.dim, *shape_args(g)]
    if entry == "bpool":
        rc = L.hipF_conv2d_backward_pooled(*head, VP(MK.ptr), MK.stride, VP(src.ptr), src.dim, pc,
                                           *tail)
    elif entry == "bpool3d":
        rc = L.hipF_conv2d_backward_pooled3d(*head, VP(MK.ptr), MK.stride, VP(src.ptr), src.dim,
                                             ph, pw, pc, *tail)
    elif entry == "backward":
        rc = L.hipF_conv2d_backward(*head, VP(src.ptr), src.dim, *tail)
    else:
        assert entry == "dgrad" and dx and not gw
        rc = L.hipF_conv2d_dgrad(VP(src.ptr), src.dim, *shape_args(g), VP(Wd.ptr), Wd.dim, g.kh,
                                 g.kw, g.G, VP(DX.ptr), DX.dim, ws[1], ws[2], VP(stream()))
    sync()
    gbh = gb.cpu().numpy()
    assert np.isnan(gbh[g.G:]).all(), "the floats after gb were written"
    return rc, DX, GW, gbh[:g.G]


def check_outputs(what, DX, GW, gb, dx, gw):
    """The present outputs; the absent ones must be as they were."""
    out = [DX.get() if dx else None, GW.get() if gw else None, gb if gw else None]
    if not dx:
        untouched(DX, f"{what}: dX (absent)")
    if not gw:
        untouched(GW, f"{what}: gW (absent)")
        assert np.isnan(gb).all(), f"{what}: gb (absent) was written"
    return out


def same_outputs(a, b, what):
    for name, u, v in zip(("dX", "gW", "gb"), a, b):
        if u is not None:
            assert_bits(u, v, f"{what}: {name}")


@pytest.mark.parametrize("case", T.select(T.BACKWARDS), ids=T.name_of)
def test_backward(kc, families, case):
    c, g = case, T.Geom(case["shape"], case["rows"])
    families(c)
    win, entry = c["win"], c["entry"]
    dx, gw = T.OUTS_ARGS[c["outs"]]
    r = rng(seed_of(c))
    x = (with_ties if c["data"] == "ties" else randn)(r, (g.R, g.CHW))
    Wm = randn(r, (g.Kdim, g.G), 1.0 / np.sqrt(g.Kdim))
    if c["data"] == "ties":
        pc = win[2]
        for j in range(g.G // pc):
            Wm[:, j * pc:(j + 1) * pc] = Wm[:, j * pc:j * pc + 1]
    X, Wd = place(kc, T.op(c, "x"), x), place(kc, T.op(c, "w"), Wm)
    MK = None
    if entry == "backward":
        dY = randn(r, (g.R, g.P * g.G))
        src = place(kc, T.op(c, "y"), dY)
    else:
        mask = make_mask(kc, c, g, r, x, Wm, X, Wd)
        assert int(mask.max()) <= PR.window_bits(win)
        if c["mask"] == "fwd":
            assert mask.min() >= 1
            assert (c["data"] == "ties") == bool((mask & (mask - 1)).any())
        dP = randn(r, (g.R, T.pooled_cols(c)))
        dY = PR.expand(mask, dP, g.G, g.oh, g.ow, win)      # a select, no arithmetic
        src = place(kc, T.op(c, "p"), dP)
        MK = MaskBuf(T.op(c, "m"), 2 if entry == "bpool3d" else 1, mask)
    rc, DX, GW, gb = run_backward(kc, c, g, X, Wd, src, MK, dx, gw)
    assert rc == 0
    got = check_outputs(c["name"], DX, GW, gb, dx, gw)
    X.get(), Wd.get(), src.get()
    if MK is not None:
        assert (MK.get() == mask).all()
    # the fixed-order reduction: a second call gives the same bits
    rc, DX2, GW2, gb2 = run_backward(kc, c, g, X, Wd, src, MK, dx, gw)
    assert rc == 0
    same_outputs(got, check_outputs("repeat", DX2, GW2, gb2, dx, gw), "repeat")
    # the unfused pair under the same families, where it runs the same arithmetic
    # (the table's field, which test_conv_pool_routes.py asserts from both calls' logs)
    if entry != "backward":
        if c["bitwise"]:
            dYm = Mat(kc, np.full((g.R, g.P * g.G), np.nan), extra=0)
            PLd = Mat(kc, dP, extra=0)
            MKd = MaskBuf((g.R, mask.shape[1], mask.shape[1], 0), 2 if entry == "bpool3d" else 1,
                          mask)
            if entry == "bpool":
                rc = kc.lib().hipF_maxpool_backprop_mask(
                    VP(MKd.ptr), MKd.stride, VP(PLd.ptr), PLd.dim, VP(dYm.ptr), dYm.dim, g.oh,
                    g.ow, win[2], VP(stream()))
            else:
                rc = kc.lib().hipF_maxpool_backprop_mask3d(
                    VP(MKd.ptr), MKd.stride, VP(PLd.ptr), PLd.dim, VP(dYm.ptr), dYm.dim, g.oh,
                    g.ow, *win, VP(stream()))
            sync()
            assert rc == 0
            assert_bits(dYm.get(), dY, "hipF_maxpool_backprop_mask vs the host's select")
            rc, DXu, GWu, gbu = run_backward(kc, c, g, X, Wd, dYm, None, dx, gw,
                                             entry="backward" if gw else "dgrad")
            assert rc == 0
            same_outputs(got, check_outputs("unfused", DXu, GWu, gbu, dx, gw),
                         "fused vs the unfused pair")
    # the oracle, on the derivative the mask routes
    oc = oracle_conv(g, Wm, np.zeros(g.G, np.float32))
    if dx:
        _, dx_t, dx_s = triple(lambda: oc.backprop(x, dY, update=False))
        assert_bound(got[0], dx_t, dx_s, what=f"{c['name']} dX")
    if gw:
        _, (gW_t, gb_t), (gW_s, gb_s) = triple(lambda: oc.gradient(x, dY))
        assert_bound(got[1], gW_t, gW_s, what=f"{c['name']} gW")
        assert_bound(got[2], gb_t, gb_s, what=f"{c['name']} gb")
    if c["mask"] == "zeros":
        assert all(v is None or (v == 0).all() for v in got), "a zero mask: exact zeros"


@pytest.mark.parametrize("case", [c for c in T.REFUSALS if "bwd misaligned declines" in c["tags"]],
                         ids=T.name_of)
def test_misaligned_bf16x6_call_declines_and_writes_nothing(kc, families, case):
    c, g = case, T.Geom(case["shape"], case["rows"])
    families(c)
    r = rng(seed_of(c))
    x, Wm = randn(r, (g.R, g.CHW)), randn(r, (g.Kdim, g.G))
    X, Wd = place(kc, T.op(c, "x"), x), place(kc, T.op(c, "w"), Wm)
    mask = np.full((g.R, T.pooled_cols(c)), 1, np.uint32)
    src = place(kc, T.op(c, "p"), randn(r, mask.shape))
    MK = MaskBuf(T.op(c, "m"), 1, mask)
    rc, DX, GW, gb = run_backward(kc, c, g, X, Wd, src, MK, True, True)
    assert rc == T.DECLINED
    untouched(DX, "dX")
    untouched(GW, "gW")
    assert np.isnan(gb).all()


def test_first_call_in_a_process(kc):
    """The first call of an f16x3 implicit-GEMM form in a process (the call that
    sets the form's dynamic-LDS attribute) succeeds: a fresh process makes it
    (tests/conv_pool_first_call.py), since this one may have made it already."""
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__),
                                                       "conv_pool_first_call.py"),
                          "ig-BG128-nopad-notab-pool1-f16"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("fused", "unfused"))]
    assert lines == ["fused rc 0", "unfused first == second True"], out.stdout
