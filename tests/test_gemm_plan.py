"""The f16x3 GEMM's plan (tile, split-K count, whole tiles in front of the
split ones; cu-gemm-f16x3.hip choose_plan) through kcnn_gemm_plan, which
needs no GPU: a pure function of the call's shape, transposes and alignment
and of the "gemm" selector."""
import ctypes

import pytest

NARROW, WIDE = 128, 256

C2_FC = [("fc_fwd", 4096, 1024, 11616, False, True),
         ("fc_dgrad", 4096, 11616, 1024, False, False),
         ("fc_wgrad", 1024, 11616, 4096, True, False)]
# the plans DESIGN.md section 3 records for c2's three FC GEMMs
C2_PLANS = {"fc_fwd": (WIDE, 4, 0), "fc_dgrad": (WIDE, 1, 0), "fc_wgrad": (NARROW, 2, 256)}

SHAPES = [(1, 1, 1), (300, 260, 77), (256, 256, 4500), (512, 256, 9024), (1024, 11616, 2048),
          (4096, 4096, 4096), (4096, 3454, 4096), (130, 70, 200), (8192, 1024, 11616),
          (16384, 11616, 1024),
          (1024, 20480, 2048), (4096, 5888, 4096)] + [c[1:4] for c in C2_FC]


@pytest.fixture
def kc():
    import kcnn
    kcnn.lib()
    old = kcnn.get_kernel_family("gemm")
    yield kcnn
    kcnn.set_kernel_family("gemm", old)


def _ws(kc, m, n, k):
    f = kc.lib().kl_gemm_f16x3_workspace_bytes
    f.restype = ctypes.c_size_t
    return int(f(m, n, k))


def _need(kc, ta, tb, m, n, k, lda, ldb):
    f = kc.lib().kl_gemm_f16x3_plan
    f.restype = ctypes.c_size_t
    out = (ctypes.c_int * 3)()
    need = int(f(int(ta), int(tb), m, n, k, lda, ldb, out))
    return need, tuple(out)


@pytest.mark.parametrize("mode", [2, 3, 4])
def test_plan_is_a_pure_function(kc, mode):
    kc.set_kernel_family("gemm", mode)
    for m, n, k in SHAPES:
        for ta in (False, True):
            for tb in (False, True):
                first = kc.gemm_plan(ta, tb, m, n, k)
                assert first[0] in (NARROW, WIDE) and first[1] >= 1 and first[2] >= 0
                assert first[2] % 256 == 0 and (first[1] > 1 or first[2] == 0)
                for _ in range(3):
                    assert kc.gemm_plan(ta, tb, m, n, k) == first
                if mode == 4:
                    assert first[0] == NARROW
                if mode == 3:   # (dense pitches: a row-contiguous operand's is M or N)
                    wide_ok = (not ta or m % 4 == 0) and (tb or n % 4 == 0)
                    assert first[0] == (WIDE if wide_ok else NARROW)
    kc.set_kernel_family("gemm", 2)


@pytest.mark.parametrize("mode", [2, 3, 4])
def test_plan_fits_the_workspace(kc, mode):
    """The workspace is sized from (M, N, K) alone, before the selector's
    value and the operands' alignment at the call are known: every plan's
    need must fit, or the launch would drop to one split."""
    kc.set_kernel_family("gemm", mode)
    for m, n, k in SHAPES:
        ws = _ws(kc, m, n, k)
        for ta in (False, True):
            for tb in (False, True):
                for pad in (0, 4, 1):
                    lda = (m if ta else k) + pad
                    ldb = (k if tb else n) + pad
                    need, plan = _need(kc, ta, tb, m, n, k, lda, ldb)
                    assert need <= ws, (m, n, k, ta, tb, pad, plan, need, ws)
                    assert (need > 0) == (plan[1] > 1)


@pytest.mark.parametrize("mode", [2, 3])
def test_unaligned_row_contiguous_operand_stays_narrow(kc, mode):
    """A row-contiguous operand (A transposed, B untransposed) whose pitch is
    no multiple of 4 takes the one-dword loader, which has no wide kernel."""
    kc.set_kernel_family("gemm", mode)
    for m, n, k in [(512, 512, 1024), (4096, 11616, 1024), (300, 260, 77)]:
        assert kc.gemm_plan(True, True, m, n, k, lda=m + 1)[0] == NARROW
        assert kc.gemm_plan(False, False, m, n, k, ldb=n + 3)[0] == NARROW
        assert kc.gemm_plan(True, False, m, n, k, lda=m + 2, ldb=n + 4)[0] == NARROW
        if mode == 3:   # K-contiguous operands' pitches do not matter to the tile
            assert kc.gemm_plan(True, False, m, n, k, lda=m + 4, ldb=n + 8)[0] == WIDE
            assert kc.gemm_plan(False, True, m, n, k, lda=k + 4, ldb=k + 4)[0] == WIDE


@pytest.mark.parametrize("name,m,n,k,ta,tb", C2_FC, ids=[c[0] for c in C2_FC])
def test_c2_plans(kc, name, m, n, k, ta, tb):
    kc.set_kernel_family("gemm", 2)
    assert kc.gemm_plan(ta, tb, m, n, k) == C2_PLANS[name]


# tests/test_gpu_gemm_fixup.py's shapes: the smallest that split K (a split's
# K / s >= 1024), with (tile, ksplit, nwhole) under selectors 2, 3 and 4.  If
# the cost model stops splitting them that file checks nothing, so this goes
# red first, without a GPU.
FIXUP_PLANS = [((256, 256, 2048), {2: (NARROW, 2, 0), 3: (WIDE, 2, 0), 4: (NARROW, 2, 0)}),
               ((260, 260, 3104), {2: (NARROW, 3, 0), 3: (WIDE, 3, 0), 4: (NARROW, 3, 0)}),
               ((256, 258, 4133), {2: (NARROW, 4, 0), 3: (WIDE, 4, 0), 4: (NARROW, 4, 0)}),
               ((260, 256, 2048), {2: (NARROW, 2, 0), 3: (WIDE, 2, 0), 4: (NARROW, 2, 0)}),
               ((1024, 11616, 2048), {2: (NARROW, 2, 256), 3: (WIDE, 1, 0),
                                      4: (NARROW, 2, 256)})]


@pytest.mark.parametrize("mode", [2, 3, 4])
@pytest.mark.parametrize("shape,plans", FIXUP_PLANS, ids=[str(p[0]) for p in FIXUP_PLANS])
def test_fixup_test_shapes_split(kc, mode, shape, plans):
    kc.set_kernel_family("gemm", mode)
    m, n, k = shape
    for ta in (False, True):
        for tb in (False, True):
            # 16-B pitches, as AddMatMat hands the operands to the kernel
            lda = (m if ta else k) + 3 & ~3
            ldb = (k if tb else n) + 3 & ~3
            assert kc.gemm_plan(ta, tb, m, n, k, lda=lda, ldb=ldb) == plans[mode]
    if mode == 2:   # the full-table case's 256 small keys
        for mi in range(4, 1025, 4):
            assert kc.gemm_plan(False, False, mi, 4, 2048) == (NARROW, 2, 0)


def test_fixup_counters_and_site_reset_need_no_gpu(kc):
    """kcnn_gemm_fixup_counts / kcnn_gemm_fixup_sites_reset are host-side: they
    work without a device, and the counters read zero after a reset."""
    kc.gemm_fixup_sites_reset()
    kc.gemm_fixup_counts(reset=True)
    assert kc.gemm_fixup_counts() == (0, 0)
    assert kc.gemm_fixup_counts(reset=True) == (0, 0)
    kc.gemm_fixup_sites_reset()
    assert kc.gemm_fixup_counts() == (0, 0)


def test_whole_plus_split_plans_on_the_wide_tile(kc):
    """The wide tile's hybrid grid (nwhole > 0) is reachable: forced on
    (1024, 20480, 2048), which tests/test_gpu_gemm_wide.py runs, and by the
    model itself on 4096 x 5888 x 4096."""
    kc.set_kernel_family("gemm", 3)
    assert kc.gemm_plan(False, True, 1024, 20480, 2048) == (WIDE, 2, 256)
    kc.set_kernel_family("gemm", 2)
    assert kc.gemm_plan(False, True, 4096, 5888, 4096) == (WIDE, 2, 256)
