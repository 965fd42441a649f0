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


def test_whole_plus_split_plans_on_the_wide_tile(kc):
    """The wide tile's hybrid grid (nwhole > 0) is reachable: forced on
    (1024, 20480, 2048), which tests/test_gpu_gemm_wide.py runs, and by the
    model itself on 4096 x 5888 x 4096."""
    kc.set_kernel_family("gemm", 3)
    assert kc.gemm_plan(False, True, 1024, 20480, 2048) == (WIDE, 2, 256)
    kc.set_kernel_family("gemm", 2)
    assert kc.gemm_plan(False, True, 4096, 5888, 4096) == (WIDE, 2, 256)
