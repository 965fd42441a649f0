"""Time maps that keep a height (frequency) axis, without a GPU: the host plan
(capi/time-plan.h with height maps) run as a stand-alone program under
AddressSanitizer and UBSan -- the (C, H, n, delta) chains of nets F and M and
of tests/golden/freq_conv.config, every decline height maps add, the
two-argument call as it always was, the row bookkeeping on utterances of (1, 7,
23, 2) frames and a host model of the whole pass against the window pass on
integer data -- and the new symbols, declared and exported.

The prefixes through kcnn_nnet_time_shared_prefix (4 for F, 9 for M, 4 for
freq_conv.config) need a network with parameters, which cannot be built
without a device (tests/test_time_plan.py): they are checked here by the
program, which parses the same configs and runs the plan NnetStack runs, and
on the networks themselves in tests/test_gpu_compute_shared_height.py."""
import ctypes
import os
import shutil
import subprocess

import kcnn
from test_abi import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("kcnn_nnet_time_map_height",)
NEW_KERNELS = ("kn_timemap_conv2d", "kn_timemap_pool2d", "kn_timemap_gather2d")


def test_time_plan_height_program_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "time_plan_height_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src"),
                    os.path.join(ROOT, "scripts", "time_plan_height_check.cc"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), os.path.join(GOLDEN, "freq_conv.config")], capture_output=True,
                       text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all time plan height checks passed" in r.stdout
    assert "net F: prefix 4, ending at (2, 5, 6, 1)" in r.stdout
    assert "net M: prefix 9, ending at (16, 1, 1, 2)" in r.stdout
    assert "freq_conv.config: prefix 4, ending at (32, 33, 11, 1)" in r.stdout
    for net in ("net F", "net M"):
        for pad in ("padded", "unpadded"):
            assert f"{net} {pad}: " in r.stdout
    assert "WRONG" not in r.stdout and "REFUSED" not in r.stdout


def test_new_symbols_declared_and_exported():
    L = _lib()
    names = kcnn.declared_symbols()
    for name in NEW:
        assert name in names, name
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "kaldi-cnn_amd", "src", "nnet2", "nnet-kernels.h")).read()
    for name in NEW_KERNELS:
        assert f"int {name}(" in header, name
        assert hasattr(L, name), name


def test_time_map_height_without_a_shared_pass_is_an_error_code():
    """No device: a network without parameters has made no shared pass."""
    L = _lib()
    L.kcnn_nnet_new.restype = ctypes.c_void_p
    h = L.kcnn_nnet_new(b"SpliceComponent input-dim=4 left-context=2 right-context=2 "
                        b"const-component-dim=0\nRectifiedLinearComponent dim=20")
    assert h, L.kcnn_last_error()
    net = ctypes.c_void_p(h)
    try:
        height = ctypes.c_int(-7)
        rc = L.kcnn_nnet_time_map_height(net, 0, ctypes.byref(height))
        assert rc != 0 and "kcnn_nnet_compute_shared" in L.kcnn_last_error().decode()
        assert height.value == -7
        rc = L.kcnn_nnet_time_map_height(net, 0, None)
        assert rc != 0 and "no result pointer" in L.kcnn_last_error().decode()
        assert L.kcnn_nnet_time_shared_prefix(net) == 0
    finally:
        L.kcnn_nnet_free(net)
