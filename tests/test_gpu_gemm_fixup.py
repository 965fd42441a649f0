"""The f16x3 GEMM's split-K recompute routes (cu-gemm-f16x3.hip), pinned
bitwise across the states of a call site's fix-up word.

With split K the store's range check runs in gemm_f16x3_reduce_kernel; a
rejected element is recomputed in fp32 by (1) the wave's own wave_dot when the
wave's 64 quads hold at most REJ_LOCAL = 4 rejections, (2) the fix-up kernel's
`rows` mode (op(B) row-contiguous and 16-B aligned, N % 4 == 0), (3) the
fix-up's other mode, or (4) the reduce itself for every rejection when the
call skipped the fix-up launch (fix_local), which it does when the previous
call at its site (M, N, K, transposes, momentum or not) deferred no group.
Which of these runs must not change a bit of C.

Every case asserts its plan (kc.gemm_plan: it really splits K) and, call by
call, whether the fix-up was launched or skipped (kc.gemm_fixup_counts after
kc.gemm_fixup_sites_reset), so no case passes without taking the route it
names; a launch after a synchronised spread call also proves that that call's
reduce met a wave with more than REJ_LOCAL rejections.  The truth is torch's
fp64 matmul on the device, the bar test_gpu_gemm.py's 1e-5 * S."""
import ctypes

import numpy as np
import pytest

from _util import assert_same, dev, host, randn, rng
from test_gpu_gemm import RTOL, _bound, _gemm_mode, _mats

pytestmark = pytest.mark.gpu

LAUNCHED, SKIPPED = (1, 0), (0, 1)
SPREAD = 28
TRANSPOSES = [(False, True), (False, False), (True, False)]


def _plan(kc, mode, ta, tb, m, n, k, **kw):
    return _gemm_mode(kc, mode, lambda: kc.gemm_plan(ta, tb, m, n, k, **kw))


def _step(torch, kc, fn, want):
    """One split-K call, synchronised (its site word is settled before the
    next launch); asserts that it launched / skipped the fix-up."""
    before = kc.gemm_fixup_counts()
    out = fn()
    torch.cuda.synchronize()
    after = kc.gemm_fixup_counts()
    got = (after[0] - before[0], after[1] - before[1])
    assert got == want, f"(launched, skipped) = {got}, expected {want}"
    return out


def _reset(kc):
    kc.gemm_fixup_sites_reset()
    kc.gemm_fixup_counts(reset=True)


def _protocol(torch, kc, spread, clean):
    """The state protocol: spread() is the call under test, clean() a call at
    the same key whose operands reject nothing.  Returns [C_a, C_b, C_c, C_d]
    of the spread call: on a fresh site (fix-up launched), after a call that
    deferred (launched), after a clean call (skipped: the reduce recomputes
    every rejection itself) and after that (launched again, which proves the
    skipped call's reduce met a wave over REJ_LOCAL)."""
    _reset(kc)
    ca = _step(torch, kc, spread, LAUNCHED)
    cb = _step(torch, kc, spread, LAUNCHED)
    _step(torch, kc, clean, LAUNCHED)
    cc = _step(torch, kc, spread, SKIPPED)
    cd = _step(torch, kc, spread, LAUNCHED)
    return [ca, cb, cc, cd]


def _eq(x, y):
    return bool(((x == y) | (x.isnan() & y.isnan())).all())


def _assert_same_bits(cs, names=("fresh", "after-deferred", "skipped", "after-skipped")):
    diff = {n: int((~((c == cs[0]) | (c.isnan() & cs[0].isnan()))).sum())
            for n, c in zip(names[1:], cs[1:]) if not _eq(c, cs[0])}
    assert not diff, f"elements whose bits differ from the {names[0]} call's: {diff}"


def _spread_operands(torch, A, B, rows=(), col=None, seed=40):
    """test_wide_spread_groups' construction on the views op(A) [M x K] and
    op(B) [K x N]: rows of op(A) of N(0,1) * 2^-28 but for one element of size
    1 whose partner row of op(B) is 0; a column of op(B) likewise with its own
    k index.  Every element of such a row or column fails the store's check."""
    k = A.shape[1]
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    k0, k1 = k // 3, k // 3 + 1
    for i0 in rows:
        A[i0] = torch.randn(k, generator=g, device="cuda") * 2.0 ** -SPREAD
        A[i0, k0] = 1.0
    if rows:
        B[k0, :] = 0.0
    if col is not None:
        B[:, col] = torch.randn(k, generator=g, device="cuda") * (0.01 * 2.0 ** -SPREAD)
        B[k1, col] = -0.01
        B[k0, col] = 0.0
        A[:, k1] = 0.0


def _gemm_calls(torch, kc, shape, ta, tb, beta, pitch=0, rows=(), col=None, inf_row=None):
    """(spread call, clean call, operands) for kc.gemm at one key; beta 1 adds
    C0 ~ N(0,1), beta 0 runs over a C filled with NaN."""
    m, n, k = shape
    a, b, c0 = _mats(torch, m, n, k, ta, tb, seed=41, pitch=pitch)
    a2, b2, _ = _mats(torch, m, n, k, ta, tb, seed=42, pitch=pitch)
    A = a.t() if ta else a
    B = b.t() if tb else b
    _spread_operands(torch, A, B, rows, col)
    if inf_row is not None:
        A[inf_row, 10] = float("inf")
    c0 = c0.clone()

    def call(x, y):
        c = c0.clone() if beta != 0.0 else torch.full_like(c0, float("nan"))
        kc.gemm(x, y, c, ta, tb, 1.0, beta)
        return c
    ref0 = c0 if beta != 0.0 else torch.zeros_like(c0)
    return (lambda: call(a, b)), (lambda: call(a2, b2)), (a, b, a2, b2, ref0)


def _bound_all(torch, cs, a, b, ref0, ta, tb, beta):
    """The bound on every distinct result (equal bits: checked once)."""
    _bound(torch, a, b, ref0, cs[0], ta, tb, 1.0, beta)
    for c in cs[1:]:
        if not torch.equal(c, cs[0]):
            _bound(torch, a, b, ref0, c, ta, tb, 1.0, beta)


def _run_states(torch, kc, mode, shape, ta, tb, beta, rows, pitch=0):
    m, n, k = shape
    spread, clean, (a, b, a2, b2, ref0) = _gemm_calls(torch, kc, shape, ta, tb, beta, pitch, rows)

    def run():
        clean_c = []
        cs = _protocol(torch, kc, spread, lambda: clean_c.append(clean()))
        return cs, clean_c[0]
    cs, cclean = _gemm_mode(kc, mode, run)
    _bound(torch, a2, b2, ref0, cclean, ta, tb, 1.0, beta)
    _bound_all(torch, cs, a, b, ref0, ta, tb, beta)
    _assert_same_bits(cs)


# (256, 256, 2048): nq = 64 quads per row, so one row of C is one wave's group
# of 64 quads: each spread row is a group of 256 rejections, deferred.
# tb = False is the fix-up's `rows` mode, tb = True its wave_dot mode.
@pytest.mark.parametrize("beta", [1.0, 0.0])
@pytest.mark.parametrize("ta,tb", TRANSPOSES + [(True, True)])
@pytest.mark.parametrize("mode,tile", [(2, 128), (3, 256), (4, 128)])
def test_states_whole_row_groups(kc, mode, tile, ta, tb, beta):
    import torch
    shape = (256, 256, 2048)
    assert _plan(kc, mode, ta, tb, *shape) == (tile, 2, 0)
    _run_states(torch, kc, mode, shape, ta, tb, beta, rows=(5, 255))


# (260, 260, 3104): nq = 65, M nq = 16900 quads in 265 groups of 64, the last
# one of 4 quads; a row's 65 quads straddle two groups.
#  - row 0 is quads 0-64: group 0 has 64 of them (256 rejections, deferred),
#    group 1 only quad 64: exactly REJ_LOCAL = 4 rejections, never deferred
#    (wave_dot in the reduce in either state);
#  - row 130 is quads 8450-8514: 62 in group 132, 3 in group 133 (12 rejections,
#    deferred beside 61 clean quads of row 131);
#  - row 259 is quads 16835-16899: 61 in group 263, and the 4 of group 264, the
#    partial last group (4 of 64 quads, 16 rejections, deferred): the fix-up's
#    lanes past `total` and the sentinel word after the last group's flag.
@pytest.mark.parametrize("beta", [1.0, 0.0])
@pytest.mark.parametrize("ta,tb", TRANSPOSES)
def test_states_straddling_and_partial_groups(kc, ta, tb, beta):
    import torch
    shape = (260, 260, 3104)
    m, n, _ = shape
    nq = (n + 3) // 4
    assert nq == 65 and (m * nq + 63) // 64 == 265 and m * nq - 264 * 64 == 4
    assert (0 * nq + 64) // 64 == 1 and (1 * nq) // 64 == 1      # group 1: row 0's quad 64 alone
    assert (259 * nq) // 64 == 263 and (259 * nq + 64) // 64 == 264
    assert _plan(kc, 2, ta, tb, *shape) == (128, 3, 0)
    _run_states(torch, kc, 2, shape, ta, tb, beta, rows=(0, 130, 259))


# (256, 258, 4133): ragged K, N % 4 != 0 with B on a 16-B pitch (258 + 2
# columns): the reduce's per-column statistics loads (bvec off) and the
# fix-up's wave_dot mode whatever the transposes; the last quad of a row has
# two columns past N.
@pytest.mark.parametrize("beta", [1.0, 0.0])
@pytest.mark.parametrize("ta,tb", TRANSPOSES)
def test_states_ragged_columns(kc, ta, tb, beta):
    import torch
    shape = (256, 258, 4133)
    m, n, k = shape
    # (AddMatMat copies an operand with an unaligned pitch to an aligned one)
    lda = 256 if ta else 4136
    ldb = 4136 if tb else 260
    assert _plan(kc, 2, ta, tb, m, n, k, lda=lda, ldb=ldb) == (128, 4, 0)
    _run_states(torch, kc, 2, shape, ta, tb, beta, rows=(5, 255), pitch=2)


def test_states_whole_plus_split_grid(kc):
    """(1024, 11616, 2048): 256 of the 364 narrow tiles run whole (their
    rejections are the tile epilogue's, in any state), the other 108 in two
    splits; spread rows 5 and 1000 cross both parts.  One case, both betas
    (under beta 1 a doubled C0 is far outside the bound; only beta 0 shows the
    last bits of a spread row's element, which C0 ~ N(0,1) rounds away)."""
    import torch
    shape = (1024, 11616, 2048)
    assert _plan(kc, 2, False, False, *shape) == (128, 2, 256)
    for beta in (1.0, 0.0):
        _run_states(torch, kc, 2, shape, False, False, beta, rows=(5, 1000))


@pytest.mark.parametrize("beta", [1.0, 0.0])
@pytest.mark.parametrize("ta,tb", TRANSPOSES)
@pytest.mark.parametrize("shape,plan,pitch", [((256, 256, 2048), (128, 2, 0), 0),
                                              ((260, 260, 3104), (128, 3, 0), 0),
                                              ((256, 258, 4133), (128, 4, 0), 2)])
def test_spread_column_only(kc, shape, plan, pitch, ta, tb, beta):
    """One spread column of op(B): one rejection per row, and 64 consecutive
    quads hold a given quad column at most once (nq >= 64), so no wave
    exceeds REJ_LOCAL: after the fresh site's first call every call skips the
    fix-up.  The bound is the proof that the rejections occurred (the
    construction fails it without the recompute); beta 0 keeps C0 from
    hiding an error of the size of the element.  In the second shape the
    column's last element, C[259][257], is in the partial last group (4 of
    its 64 quads exist), whose wave must still recompute it with all of its
    lanes: wave_dot spreads K over the 64 lanes."""
    import torch
    m, n, k = shape
    kw = dict(lda=256 if ta else 4136, ldb=4136 if tb else 260) if pitch else {}
    assert _plan(kc, 2, ta, tb, m, n, k, **kw) == plan
    spread, _, (a, b, _, _, ref0) = _gemm_calls(torch, kc, shape, ta, tb, beta, pitch, col=n - 3)

    def run():
        _reset(kc)
        return [_step(torch, kc, spread, LAUNCHED), _step(torch, kc, spread, SKIPPED),
                _step(torch, kc, spread, SKIPPED)]
    cs = _gemm_mode(kc, 2, run)
    _bound_all(torch, cs, a, b, ref0, ta, tb, beta)
    _assert_same_bits(cs, ("fresh", "second", "third"))


@pytest.mark.parametrize("beta", [1.0, 0.0])
@pytest.mark.parametrize("ta,tb", TRANSPOSES)
@pytest.mark.parametrize("shape,rows,inf_row", [((256, 256, 2048), (5, 255), 77),
                                                ((260, 260, 3104), (0, 130, 259), 131)])
def test_spread_row_crossing_column_with_inf_row(kc, shape, rows, inf_row, ta, tb, beta):
    """Spread rows crossing a spread column, and an Inf row of op(A) (the
    epilogue's, split 0) in the same call: sgemm's IEEE pattern as
    test_gemm_nonfinite_pattern asserts it, the bound on the finite part, and
    the same bits in every state."""
    import torch
    m, n, k = shape
    assert _plan(kc, 2, ta, tb, m, n, k)[1] > 1
    spread, clean, (a, b, _, _, c0) = _gemm_calls(torch, kc, shape, ta, tb, beta, rows=rows,
                                                  col=n - 3, inf_row=inf_row)
    cs = _gemm_mode(kc, 2, lambda: _protocol(torch, kc, spread, clean))
    A = (a.t() if ta else a).double()
    B = (b.t() if tb else b).double()
    t = A @ B + beta * c0.double()
    fin = torch.isfinite(t)
    assert int((~fin).sum()) >= n - 1          # the Inf row
    s = A.abs().nan_to_num(posinf=0) @ B.abs().nan_to_num(posinf=0) + beta * c0.double().abs()
    for c in cs:
        assert torch.equal(torch.isnan(c), torch.isnan(t))
        assert torch.equal(torch.isposinf(c), torch.isposinf(t))
        assert torch.equal(torch.isneginf(c), torch.isneginf(t))
        err = (c.double() - t).abs()[fin]
        assert float((err / s[fin].clamp_min(1e-300)).max()) <= RTOL
    _assert_same_bits(cs)


def test_full_site_table(kc):
    """With all 256 sites taken a further key has no word: every call at it
    launches the fix-up, clean or spread, with the bits of a fresh site."""
    import torch
    shape, ta, tb = (256, 256, 2048), False, False
    spread, clean, (a, b, a2, b2, ref0) = _gemm_calls(torch, kc, shape, ta, tb, 1.0,
                                                      rows=(5, 255))

    def run():
        assert kc.gemm_plan(ta, tb, *shape)[1] == 2
        _reset(kc)
        fresh = _step(torch, kc, spread, LAUNCHED)
        _reset(kc)
        g = torch.Generator(device="cuda")
        g.manual_seed(43)
        x = torch.randn((1024, 2048), generator=g, device="cuda")
        y = torch.randn((2048, 4), generator=g, device="cuda") * 0.01
        for i in range(256):
            mi = 4 * (i + 1)
            assert kc.gemm_plan(False, False, mi, 4, 2048)[1] == 2, mi
            _step(torch, kc, lambda: kc.gemm(x[:mi], y, torch.empty((mi, 4), device="cuda")),
                  LAUNCHED)
        try:
            cclean = _step(torch, kc, clean, LAUNCHED)
            c1 = _step(torch, kc, spread, LAUNCHED)
            _step(torch, kc, clean, LAUNCHED)
            c2 = _step(torch, kc, spread, LAUNCHED)
            # (a registered site still skips after a clean call)
            _step(torch, kc, lambda: kc.gemm(x[:4], y, torch.empty((4, 4), device="cuda")),
                  SKIPPED)
        finally:
            _reset(kc)
        return fresh, cclean, c1, c2
    fresh, cclean, c1, c2 = _gemm_mode(kc, 2, run)
    _bound(torch, a2, b2, ref0, cclean, ta, tb, 1.0, 1.0)
    _bound_all(torch, [fresh, c1, c2], a, b, ref0, ta, tb, 1.0)
    _assert_same_bits([fresh, c1, c2], ("fresh", "full-table", "full-table again"))


def test_fc_bias_in_fixup_store(kc):
    """FullyConnectedComponent Propagate, 2048 -> 256 on 260 frames of which
    two are spread rows: the bias is added in the store of whichever route
    recomputes them.  Bitwise CopyRowsFromVec(bias) then kc.gemm(beta = 1)
    (test_fc_bias_in_gemm_store), each in both states; the two share one site
    (the bias is not part of the key)."""
    import torch
    I, Od, N = 2048, 256, 260
    assert kc.gemm_plan(False, True, N, Od, I)[1] == 2
    comp = kc.Component.NewFromString(
        f"FullyConnectedComponent input-dim={I} output-dim={Od} learning-rate=0.02 "
        f"param-stddev=0.01 bias-stddev=1")
    r = rng(I + Od + 1)
    W = dev(randn(r, (Od, I), 0.05))
    bias = randn(r, (Od,), 0.5)
    bias[::2] = 0.0     # (a spread row's element is ~1e-9: a bias of 0.5 rounds its last bits away)
    x = dev(randn(r, (N, I)))
    x2 = dev(randn(r, (N, I)))
    _spread_operands(torch, x, W.t(), rows=(3, 258))
    comp.SetParam(0, W)
    comp.SetParam(1, dev(bias))

    def ref(inp):
        c = dev(np.broadcast_to(bias, (N, Od)).copy())
        kc.gemm(inp, W, c, False, True, 1.0, 1.0)
        return c
    _reset(kc)
    ya = _step(torch, kc, lambda: comp.Propagate(x), LAUNCHED)
    ca = _step(torch, kc, lambda: ref(x), LAUNCHED)
    _step(torch, kc, lambda: ref(x2), LAUNCHED)
    yc = _step(torch, kc, lambda: comp.Propagate(x), SKIPPED)
    _step(torch, kc, lambda: comp.Propagate(x2), LAUNCHED)
    cc = _step(torch, kc, lambda: ref(x), SKIPPED)
    b0 = dev(np.broadcast_to(bias, (N, Od)).copy())
    _bound(torch, x, W, b0, ya, False, True, 1.0, 1.0)
    _assert_same_bits([ya, ca, yc, cc], ("Propagate launched", "gemm launched",
                                        "Propagate skipped", "gemm skipped"))


class _Raw:
    """kl_gemm_f16x3, kl_gemm_f16x3_momentum and hipF_momentum_update through
    ctypes (a handle of its own: its argtypes stay out of kcnn.py's)."""

    def __init__(self, kc, torch, m, n, k):
        self.torch = torch
        self.L = L = ctypes.CDLL(kc.LIB_PATH)
        L.kl_gemm_f16x3_full_workspace_bytes.restype = ctypes.c_size_t
        self.wsb = int(L.kl_gemm_f16x3_full_workspace_bytes(m, n, k))
        self.ws = torch.empty(self.wsb // 4 + 4, dtype=torch.int32, device="cuda")
        self.m, self.n, self.k = m, n, k
        vp, f, i = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
        L.kl_gemm_f16x3.argtypes = [i, i, i, i, i, f, vp, i, vp, i, f, vp, i, vp,
                                    ctypes.c_size_t, vp]
        L.kl_gemm_f16x3_momentum.argtypes = [i, i, i, i, i, vp, i, vp, i, vp, vp, vp, i, vp, i,
                                             f, f, f, vp, ctypes.c_size_t, vp]
        D = kc.MatrixDim
        L.hipF_momentum_update.argtypes = [vp, D, vp, D, vp, D, f, f, f, vp, vp, i, vp]
        self.D = D

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def fused(self, a, b, ta, tb, W, prev, mom, a_wd, a_g):
        rc = self.L.kl_gemm_f16x3_momentum(int(ta), int(tb), self.m, self.n, self.k, a.data_ptr(),
                                           a.stride(0), b.data_ptr(), b.stride(0), None, None,
                                           W.data_ptr(), W.stride(0), prev.data_ptr(),
                                           prev.stride(0), mom, a_wd, a_g, self.ws.data_ptr(),
                                           self.wsb, self._stream())
        assert rc == 0, rc

    def gradient(self, a, b, ta, tb, g):
        rc = self.L.kl_gemm_f16x3(int(ta), int(tb), self.m, self.n, self.k, 1.0, a.data_ptr(),
                                  a.stride(0), b.data_ptr(), b.stride(0), 0.0, g.data_ptr(),
                                  g.stride(0), self.ws.data_ptr(), self.wsb, self._stream())
        assert rc == 0, rc

    def update(self, W, prev, g, mom, a_wd, a_g):
        dims = [self.D(t.shape[0], t.shape[1], t.stride(0)) for t in (W, prev, g)]
        rc = self.L.hipF_momentum_update(W.data_ptr(), dims[0], prev.data_ptr(), dims[1],
                                         g.data_ptr(), dims[2], mom, a_wd, a_g, None, None, 0,
                                         self._stream())
        assert rc == 0, rc


@pytest.mark.parametrize("unfused_state", [LAUNCHED, SKIPPED], ids=["unfused-launched",
                                                                   "unfused-skipped"])
@pytest.mark.parametrize("fused_state", [LAUNCHED, SKIPPED], ids=["fused-launched",
                                                                 "fused-skipped"])
@pytest.mark.parametrize("ta,tb", [(True, False), (False, True)])
@pytest.mark.parametrize("shape,rows", [((256, 256, 2048), (5, 255)),
                                        ((260, 260, 3104), (0, 130, 259))])
def test_momentum_in_fixup_store(kc, shape, rows, ta, tb, fused_state, unfused_state):
    """kl_gemm_f16x3_momentum (the update applied in the store of whichever
    route recomputes a rejected element) against kl_gemm_f16x3 (alpha 1, beta
    0) into a buffer followed by hipF_momentum_update: bitwise, in all four
    combinations of the two calls' states (they are different sites: momentum
    is part of the key), and both against the fp64 formula of momentum-step.h,
    prev' = m prev + a_wd W + a_g g, W' = W + prev', within 1e-5 of the sum of
    the terms' magnitudes (the gradient's being |a_g| S)."""
    import torch
    m, n, k = shape
    assert kc.gemm_plan(ta, tb, m, n, k)[1] > 1
    a, b, _ = _mats(torch, m, n, k, ta, tb, seed=51)
    a2, b2, _ = _mats(torch, m, n, k, ta, tb, seed=52)
    _spread_operands(torch, a.t() if ta else a, b.t() if tb else b, rows)
    g0 = torch.Generator(device="cuda")
    g0.manual_seed(53)
    W0 = torch.randn((m, n), generator=g0, device="cuda") * 0.05
    P0 = torch.randn((m, n), generator=g0, device="cuda") * 0.01
    # half of each spread row starts at W = prev = 0, so prev' = W' = a_g g
    # keeps the gradient's last bits (elsewhere prev ~ 0.01 rounds them away)
    for i0 in rows:
        W0[i0, ::2] = 0.0
        P0[i0, ::2] = 0.0
    mom, a_wd, a_g = 0.9, -4e-6, 1e-3
    raw = _Raw(kc, torch, m, n, k)

    def fused(x, y):
        W, P = W0.clone(), P0.clone()
        raw.fused(x, y, ta, tb, W, P, mom, a_wd, a_g)
        return W, P

    def unfused(x, y):
        W, P, g = W0.clone(), P0.clone(), torch.full_like(W0, float("nan"))
        raw.gradient(x, y, ta, tb, g)
        raw.update(W, P, g, mom, a_wd, a_g)
        return W, P
    _reset(kc)
    # each site's word: a clean call clears it (the next call skips), a spread
    # call sets it (the next call launches)
    for call, state in ((fused, fused_state), (unfused, unfused_state)):
        if state == SKIPPED:
            _step(torch, kc, lambda: call(a2, b2), LAUNCHED)
        else:
            _step(torch, kc, lambda: call(a, b), LAUNCHED)
    Wf, Pf = _step(torch, kc, lambda: fused(a, b), fused_state)
    Wu, Pu = _step(torch, kc, lambda: unfused(a, b), unfused_state)
    A = (a.t() if ta else a).double()
    B = (b.t() if tb else b).double()
    gt, gs = A @ B, A.abs() @ B.abs()
    pt = mom * P0.double() + a_wd * W0.double() + a_g * gt
    ps = (mom * P0.double()).abs() + (a_wd * W0.double()).abs() + abs(a_g) * gs
    wt, wsc = W0.double() + pt, ps + W0.double().abs()
    for what, got, t, s in (("prev' fused", Pf, pt, ps), ("W' fused", Wf, wt, wsc),
                            ("prev' unfused", Pu, pt, ps), ("W' unfused", Wu, wt, wsc)):
        assert torch.isfinite(got).all(), what
        worst = float(((got.double() - t).abs() / s.clamp_min(1e-300)).max())
        assert worst <= RTOL, f"{what}: max err/S {worst:.3e}"
    assert torch.equal(Pf, Pu), f"prev': {int((Pf != Pu).sum())} elements differ"
    assert torch.equal(Wf, Wu), f"W': {int((Wf != Wu).sum())} elements differ"


@pytest.mark.parametrize("fused_state", [LAUNCHED, SKIPPED], ids=["fused-launched",
                                                                 "fused-skipped"])
def test_fc_update_across_site_states(kc, fused_state):
    """FullyConnectedComponent 256 -> 256 on 2048 frames with two spread
    derivative columns (test_fc_update_equals_gradient_then_apply's): the
    update fused into Backprop's weight-gradient GEMM against ComputeGradient
    + ApplyGradient, with the two GEMMs' sites in opposite states."""
    import torch
    I = Od = 256
    N = 2048
    assert kc.gemm_plan(True, False, Od, I, N)[1] == 2
    unfused_state = SKIPPED if fused_state == LAUNCHED else LAUNCHED
    line = (f"FullyConnectedComponent input-dim={I} output-dim={Od} learning-rate=0.02 "
            f"param-stddev=0.01 bias-stddev=1 weight-decay=0.0002 momentum=0.9")
    r = rng(19)
    params = [randn(r, (Od, I), 0.05), randn(r, (Od,), 0.5), randn(r, (Od, I), 0.01)]
    xh, dyh = randn(r, (N, I)), randn(r, (N, Od), 0.1)
    x2, dy2 = dev(xh.copy()), dev(dyh.copy())
    k0 = N // 3
    for j0 in (3, Od - 2):
        dyh[:, j0] = randn(r, (N,), 2.0 ** -SPREAD)
        dyh[k0, j0] = 1.0
    xh[k0, :] = 0.0
    for j0 in (3, Od - 2):      # (half of each spread gradient row: W' = prev' = a_g g)
        params[0][j0, ::2] = 0.0
        params[2][j0, ::2] = 0.0
    x, dy = dev(xh), dev(dyh)

    def comp():
        c = kc.Component.NewFromString(line)
        for which, v in enumerate(params):
            c.SetParam(which, dev(v))
        return c

    def fused(xx, dd):
        c = comp()
        c.Backprop(xx, None, dd, update=True)
        return [host(c.GetParam(w)) for w in range(3)]

    def unfused(xx, dd):
        c = comp()
        c.ApplyGradient(c.ComputeGradient(xx, dd), N)
        return [host(c.GetParam(w)) for w in range(3)]
    _reset(kc)
    for call, state in ((fused, fused_state), (unfused, unfused_state)):
        if state == SKIPPED:
            _step(torch, kc, lambda: call(x2, dy2), LAUNCHED)
        else:
            _step(torch, kc, lambda: call(x, dy), LAUNCHED)
    pf = _step(torch, kc, lambda: fused(x, dy), fused_state)
    pu = _step(torch, kc, lambda: unfused(x, dy), unfused_state)
    for w in range(3):
        assert_same(pf[w], pu[w], f"FC param {w}")
