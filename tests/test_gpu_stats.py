"""The f16x3 GEMM's own operand statistics (kaldi-lite/cu-f16-stats.hip:
stats_kernel, stats_finalize_kernel, stats_count_kernel) through their four
entry points kl_absmax_rows, kl_absmax_cols, kl_absmax_rows_cols and
kl_gemm_stats3, bit for bit against the numpy definition of a statistics
block (tests/f16_stats_ref.py; tests/test_f16_stats_ref.py holds that
definition to hand-written groups).

Every input is pitched and its padding is NaN, so a read past a row shows as
a maximum of 0x7fc00000; every output is followed by 64 guard words.  Each
shape is run on three kinds of data -- plain, special (zero, single-element,
NaN, +-Inf, subnormal and negative / -0.0 groups) and spread (groups of
N(0,1) 2^-28 around one element of size 1, groups on either side of the
20-binade rule and of the small-element bound).  A shape with fewer groups
than a kind has group recipes gets several matrices, so that every recipe
meets every shape.

The combined launches are compared with the separate ones, which are
themselves held to the numpy definition here.
"""
import ctypes

import numpy as np
import pytest

from _util import rng
from f16_stats_ref import stats_parts

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
GUARD = 64
P = ctypes.c_void_p
I = ctypes.c_int


@pytest.fixture(scope="module")
def L(kc):
    lib = kc.lib()
    lib.kl_absmax_rows.argtypes = [P, I, I, I, P, P]
    lib.kl_absmax_rows.restype = I
    lib.kl_absmax_cols_words.argtypes = [I, I]
    lib.kl_absmax_cols_words.restype = ctypes.c_size_t
    lib.kl_absmax_cols.argtypes = [P, I, I, I, P, P, P]
    lib.kl_absmax_cols.restype = I
    lib.kl_absmax_rows_cols.argtypes = [P, I, I, I, P, P, I, I, I, P, P, P, P]
    lib.kl_absmax_rows_cols.restype = I
    lib.kl_gemm_stats3.argtypes = [P, I, I, I, I, P, P] * 3 + [P, P]
    lib.kl_gemm_stats3.restype = I
    return lib


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


# ---- device buffers ------------------------------------------------------------
class Pitched:
    """x on the device with row pitch ld, `offset` floats into its
    allocation; everything that is not an element of x is NaN."""

    def __init__(self, x, ld, offset=0):
        import torch
        rows, cols = x.shape
        assert ld >= cols
        self.rows, self.cols, self.ld = rows, cols, ld
        h = np.full(offset + max(rows, 1) * ld, np.nan, np.float32)
        h[offset:offset + rows * ld].reshape(rows, ld)[:, :cols] = x
        self.t = torch.from_numpy(h).cuda()
        self.ptr = self.t.data_ptr() + 4 * offset


def aligned_ld(cols):
    """The smallest pitch above cols that keeps rows 16-B aligned."""
    return (cols // 4 + 1) * 4


class Words:
    """n uint32 words holding the sentinel, followed by guard words."""

    def __init__(self, n, guard=GUARD):
        import torch
        self.n = n
        self.t = torch.full((n + guard,), SENT, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr()

    def get(self):
        a = self.t.cpu().numpy().view(np.uint32)
        assert (a[self.n:] == SENT).all(), "guard words after the block were written"
        return a[:self.n]


def scratch(L, rows, cols):
    """The column form's partials.  Their guard is four rows of partials
    longer, so that a finalize pass that takes a row chunk too many reads the
    sentinel (and gives a wrong minimum) instead of another allocation."""
    return Words(L.kl_absmax_cols_words(rows, cols), GUARD + 4 * cols)


def check_parts(got, x, axis, what):
    """got: a block of 3 n words; x: the matrix; equality with the definition,
    naming the part and the first differing groups."""
    want = stats_parts(x, axis)
    n = want[0].size
    assert got.size == 3 * n, (what, got.size, n)
    for k, part in enumerate(("max", "min", "cnt")):
        g, e = got[k * n:(k + 1) * n], want[k]
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, (f"{what}: {part} differs at {bad[:5]}: "
                               f"got {[hex(v) for v in g[bad[:5]]]} want {[hex(v) for v in e[bad[:5]]]}")


def run_rows(L, x, ld=None, offset=0):
    X = Pitched(x, aligned_ld(x.shape[1]) if ld is None else ld, offset)
    out = Words(3 * X.rows)
    rc = L.kl_absmax_rows(X.ptr, X.rows, X.cols, X.ld, out.ptr, stream())
    sync()
    assert rc == 0
    return out.get()


def run_cols(L, x, ld=None, offset=0):
    X = Pitched(x, aligned_ld(x.shape[1]) if ld is None else ld, offset)
    out = Words(3 * X.cols)
    part = scratch(L, X.rows, X.cols)
    assert part.n > 0
    rc = L.kl_absmax_cols(X.ptr, X.rows, X.cols, X.ld, out.ptr, part.ptr, stream())
    sync()
    assert rc == 0
    part.get()  # (its guard)
    return out.get()


# ---- data ----------------------------------------------------------------------
def f32(v):
    return np.asarray(v, np.float32)


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def group_of(r, n, first, fill):
    """A group of n elements: `first` (truncated to n), then fill(k) values,
    in a random order (so that the marked elements land in any tail)."""
    first = f32(first)[:n]
    g = np.concatenate([first, f32(fill(n - first.size))])
    return g[r.permutation(n)]


def randn_fill(r, scale=1.0):
    return lambda k: r.standard_normal(k) * scale


def between(r, lo_exp, hi_exp):
    """fill: random signs, magnitudes in [2^lo_exp, 2^hi_exp)"""
    def fill(k):
        e = r.integers(lo_exp, hi_exp, size=k)
        return np.ldexp(r.uniform(1.0, 2.0, size=k), e) * r.choice([-1.0, 1.0], size=k)
    return fill


def special_recipes(r, n):
    sub = lambda k: from_bits(r.integers(1, 0x800000, size=k).astype(np.uint32)
                              | (r.integers(0, 2, size=k).astype(np.uint32) << 31))
    return [
        lambda: np.zeros(n, np.float32),                                 # a zero group
        lambda: group_of(r, n, [r.standard_normal()], np.zeros),         # a single nonzero element
        lambda: group_of(r, n, [np.nan], randn_fill(r)),
        lambda: group_of(r, n, [np.inf], randn_fill(r)),
        lambda: group_of(r, n, [-np.inf], randn_fill(r)),
        lambda: group_of(r, n, [], sub),                                 # subnormals only
        lambda: group_of(r, n, [-0.0, -0.0], lambda k: -np.abs(r.standard_normal(k)) - 1e-3),
    ]


def spread_recipes(r, n):
    at = f32(2.0 ** -14)                       # small_bound of a max in [8, 16)
    below = from_bits(at.view(np.uint32) - 1)  # one ulp under it
    tiny = randn_fill(r, 2.0 ** -28)
    return [
        lambda: group_of(r, n, [1.0], tiny),
        lambda: group_of(r, n, [-1.0], tiny),
        lambda: group_of(r, n, [1.0], tiny),
        # min exactly 20 binades under the max: not spread
        lambda: group_of(r, n, [1.5 * 2.0 ** 3, -1.25 * 2.0 ** -17], between(r, -16, 3)),
        # exactly 21 under: spread, and the min is its only small element
        lambda: group_of(r, n, [-1.5 * 2.0 ** 3, 1.99 * 2.0 ** -18], between(r, -14, 3)),
        # at the small-element bound (not counted) and one ulp below (counted)
        lambda: group_of(r, n, [9.0, 2.0 ** -30, at, -at, below, -below, below],
                         between(r, -14, 3)),
    ]


def datasets(kind, ngroups, glen, seed):
    """Group-major matrices [ngroups x glen] of one kind of data: as many as
    it takes for every recipe to appear."""
    r = rng(seed)
    if kind == "plain":
        return [f32(r.standard_normal((ngroups, glen)))]
    recipes = (special_recipes if kind == "special" else spread_recipes)(r, glen)
    K = len(recipes)
    if ngroups >= K:
        # one matrix: the recipes on groups from the first to the last, the
        # other groups plain
        m = f32(r.standard_normal((ngroups, glen)))
        for k in range(K):
            m[k * (ngroups - 1) // (K - 1)] = recipes[k]()
        return [m]
    out = []
    for v in range(-(-K // ngroups)):
        m = f32(r.standard_normal((ngroups, glen)))
        for g in range(ngroups):
            if v * ngroups + g < K:
                m[g] = recipes[v * ngroups + g]()
        out.append(m)
    return out


def spread_census(mats):
    """(spread groups with cnt > 1, groups that are not spread) over
    group-major matrices, by the definition alone."""
    many = plain = 0
    for m in mats:
        mx, mn, cnt = stats_parts(m, 1)
        many += int((cnt > 1).sum())
        # cnt is 0 exactly when a group is not spread (a spread group's
        # minimum is one of its small elements)
        plain += int((cnt == 0).sum())
    return many, plain


def sweep(L, form, shapes, kind, seed):
    """Every shape on one kind of data, rows x cols with the groups along
    `form`."""
    run = run_rows if form == "rows" else run_cols
    for i, (rows, cols) in enumerate(shapes):
        ngroups, glen = (rows, cols) if form == "rows" else (cols, rows)
        mats = datasets(kind, ngroups, glen, seed + i)
        # (a group of one or two elements cannot hold a count above 1)
        if kind == "spread" and glen >= 3:
            many, plain = spread_census(mats)
            assert many >= 1 and plain >= 1, (rows, cols, many, plain)
        for v, m in enumerate(mats):
            x = np.ascontiguousarray(m if form == "rows" else m.T)
            assert x.shape == (rows, cols)
            check_parts(run(L, x), x, 1 if form == "rows" else 0,
                        f"{form} {rows} x {cols} {kind} #{v}")


KINDS = ["plain", "special", "spread"]

ROW_CASES = {
    # a wave per row: the r >= rows exit, quad tails
    "wave": [(r, c) for r in (1, 3, 4, 5, 9) for c in (1, 3, 4, 5, 255, 256, 257, 1025, 2047)],
    # a block per row, the row held in registers up to 18432 floats
    "block_held": [(3, 2048), (3, 2049), (2, 4611), (2, 18432)],
    # past that: the 4-in-flight loop, its scalar tail, count_small_row
    "block_not_held": [(2, 18436), (2, 20483)],
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(ROW_CASES))
def test_rows(L, case, kind):
    sweep(L, "rows", ROW_CASES[case], kind, 1000 * len(case) + len(kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("offset", [0, 1])
def test_rows_unaligned(L, offset, kind):
    """ld = cols + 1 (5 x 257: rows off 16 B; 2 x 2051: ld 2052, aligned until
    the base moves by one float): the vec == 0 sweeps."""
    for i, (rows, cols) in enumerate([(5, 257), (2, 2051)]):
        mats = datasets(kind, rows, cols, 70 + 10 * offset + i)
        if kind == "spread":
            many, plain = spread_census(mats)
            assert many >= 1 and plain >= 1, (rows, cols, many, plain)
        for v, x in enumerate(mats):
            got = run_rows(L, x, ld=cols + 1, offset=offset)
            check_parts(got, x, 1, f"rows {rows} x {cols} ld {cols + 1} offset {offset} {kind} #{v}")


COL_CASES = {
    # the 8-in-flight row loop and its tail, the last quad of columns
    "row_tails": [(r, c) for r in (1, 7, 8, 9, 15, 16, 17) for c in (1, 3, 4, 5, 63, 64, 65)],
    "two_column_blocks": [(40, 1023), (40, 1024), (40, 1025)],
    # the count kernel's 64-row chunks: the spread columns' small elements
    # lie in every chunk (all but one element of such a column is small)
    "count_chunks": [(64, 70), (65, 70), (130, 70)],
    # the finalize's 8-in-flight loop (29 and more row chunks), rbk = 256
    "many_row_chunks": [(464, 70), (500, 130), (4100, 70)],
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(COL_CASES))
def test_cols(L, case, kind):
    sweep(L, "cols", COL_CASES[case], kind, 2000 * len(case) + len(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_cols_unaligned(L, kind):
    mats = datasets(kind, 66, 33, 90)
    if kind == "spread":
        many, plain = spread_census(mats)
        assert many >= 1 and plain >= 1, (many, plain)
    for v, m in enumerate(mats):
        x = np.ascontiguousarray(m.T)
        check_parts(run_cols(L, x, ld=67), x, 0, f"cols 33 x 66 ld 67 {kind} #{v}")


def test_count_chunks_cover_every_chunk(L):
    """A spread column of 130 rows with exactly one small element, placed in
    each 64-row chunk in turn and on the chunks' edges."""
    r = rng(5)
    places = [0, 63, 64, 127, 128, 129]
    x = f32(np.ldexp(r.uniform(1.0, 2.0, size=(130, 70)), 0))
    for c, row in enumerate(places):
        x[row, c] = 2.0 ** -30
    mx, mn, cnt = stats_parts(x, 0)
    assert cnt[:len(places)].tolist() == [1] * len(places) and cnt[len(places):].sum() == 0
    check_parts(run_cols(L, x), x, 0, "cols 130 x 70, one small element per column")


# ---- combined launches ----------------------------------------------------------
def operands(seed):
    """A row operand and a column operand from the lists above, spread data."""
    R = datasets("spread", 9, 1025, seed)[0]
    Q = np.ascontiguousarray(datasets("spread", 70, 130, seed + 1)[0].T)
    return R, Q


@pytest.mark.parametrize("with_clear", [True, False])
def test_rows_cols(L, with_clear):
    R, Q = operands(300)
    rows_sep, cols_sep = run_rows(L, R), run_cols(L, Q)
    check_parts(rows_sep, R, 1, "separate rows")
    check_parts(cols_sep, Q, 0, "separate cols")
    XR, XQ = Pitched(R, aligned_ld(R.shape[1])), Pitched(Q, aligned_ld(Q.shape[1]))
    ro, co = Words(3 * XR.rows), Words(3 * XQ.cols)
    part = scratch(L, XQ.rows, XQ.cols)
    clear = Words(2)
    rc = L.kl_absmax_rows_cols(XR.ptr, XR.rows, XR.cols, XR.ld, ro.ptr,
                               XQ.ptr, XQ.rows, XQ.cols, XQ.ld, co.ptr, part.ptr,
                               clear.ptr if with_clear else None, stream())
    sync()
    assert rc == 0
    part.get()
    assert (ro.get() == rows_sep).all(), "rows differ from kl_absmax_rows"
    assert (co.get() == cols_sep).all(), "columns differ from kl_absmax_cols"
    assert clear.get().tolist() == ([0, 0] if with_clear else [SENT, SENT])


@pytest.mark.parametrize("skip", [None, 0, 1, 2])
def test_gemm_stats3(L, skip):
    X0 = np.ascontiguousarray(datasets("spread", 70, 130, 310)[0].T)      # 130 x 70
    X2 = np.ascontiguousarray(datasets("spread", 1025, 40, 311)[0].T)     # 40 x 1025
    sep = [run_rows(L, X0), run_cols(L, X0), run_cols(L, X2)]
    check_parts(sep[0], X0, 1, "separate rows of X0")
    check_parts(sep[1], X0, 0, "separate cols of X0")
    check_parts(sep[2], X2, 0, "separate cols of X2")
    D0, D2 = Pitched(X0, aligned_ld(70)), Pitched(X2, aligned_ld(1025))
    ops = [(D0, 0), (D0, 1), (D2, 1)]
    outs = [Words(3 * (d.rows if mode == 0 else d.cols)) for d, mode in ops]
    parts = [scratch(L, d.rows, d.cols) if mode else None for d, mode in ops]
    args = []
    for i, (d, mode) in enumerate(ops):
        args += [None if i == skip else d.ptr, d.rows, d.cols, d.ld, mode, outs[i].ptr,
                 parts[i].ptr if parts[i] else None]
    rc = L.kl_gemm_stats3(*args, None, stream())
    sync()
    assert rc == 0
    for i in range(3):
        got = outs[i].get()
        if parts[i]:
            parts[i].get()
        if i == skip:
            assert (got == SENT).all(), f"skipped operand {i}'s output was written"
        else:
            assert (got == sep[i]).all(), f"operand {i} differs from its separate launch"


def test_empty_operands(L):
    X = Pitched(f32(np.ones((4, 8))), 8)
    for rows, cols in ((0, 5), (3, 0)):
        out = Words(3 * rows)
        assert L.kl_absmax_rows(X.ptr, rows, cols, 8, out.ptr, stream()) == 0
        sync()
        assert (out.get() == 0).all(), ("rows", rows, cols)
        out = Words(3 * cols)
        assert L.kl_absmax_cols_words(rows, cols) == 0
        assert L.kl_absmax_cols(X.ptr, rows, cols, 8, out.ptr, None, stream()) == 0
        sync()
        assert (out.get() == 0).all(), ("cols", rows, cols)


def test_rejected_arguments(L):
    """Host checks, no launch: nonzero, and the output keeps its sentinel."""
    X = Pitched(f32(np.ones((4, 8))), 8)
    out, part = Words(3 * 8), Words(L.kl_absmax_cols_words(4, 8))
    s = stream()
    assert L.kl_absmax_rows(X.ptr, 4, 8, 7, out.ptr, s) != 0            # ld < cols
    assert L.kl_absmax_rows(X.ptr, 4, 8, 8, None, s) != 0               # no output
    assert L.kl_absmax_cols(X.ptr, 4, 8, 7, out.ptr, part.ptr, s) != 0
    assert L.kl_absmax_cols(X.ptr, 4, 8, 8, None, part.ptr, s) != 0
    assert L.kl_absmax_cols(X.ptr, 4, 8, 8, out.ptr, None, s) != 0      # column form, no part
    assert L.kl_absmax_rows_cols(X.ptr, 4, 8, 8, out.ptr, X.ptr, 4, 8, 8, out.ptr, None,
                                 None, s) != 0
    assert L.kl_gemm_stats3(X.ptr, 4, 8, 8, 1, out.ptr, None, None, 0, 0, 0, 0, None, None,
                            None, 0, 0, 0, 0, None, None, None, s) != 0
    assert L.kl_gemm_stats3(X.ptr, 4, 8, 7, 0, out.ptr, None, None, 0, 0, 0, 0, None, None,
                            None, 0, 0, 0, 0, None, None, None, s) != 0
    sync()
    assert (out.get() == SENT).all() and (part.get() == SENT).all()
