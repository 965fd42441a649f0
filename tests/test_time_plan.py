"""The time-shared whole-utterance forward, without a GPU: the host plan
(capi/time-plan.h) run as a stand-alone program under AddressSanitizer and
UBSan -- the golden configs' prefixes and (C, n, delta) chains, every decline,
the row bookkeeping and a host model of the pass against the window pass --
and the new C entry points: declared, exported, and refusing what
kcnn_nnet_compute refuses with an error code and a message before any device
is touched (the networks below own no device memory; a network with
parameters cannot be built without a device, so the prefixes of the golden
configs and of nets C, D and E through kcnn_nnet_time_shared_prefix are in
test_gpu_compute_shared.py, and here in the program, which parses the configs
itself)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import kcnn
from test_abi import _lib
from test_compute_abi import CONFIG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("kcnn_nnet_compute_shared", "kcnn_nnet_time_shared_prefix", "kcnn_nnet_time_map")


def test_time_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "time_plan_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src"),
                    os.path.join(ROOT, "scripts", "time_plan_check.cc"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), os.path.join(GOLDEN, "nnet.config"),
                        os.path.join(GOLDEN, "train_conv.config")], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all time plan checks passed" in r.stdout
    assert "nnet.config: prefix 14, ending at (512, 2, 2)" in r.stdout
    assert "train_conv.config: prefix 4, ending at (128, 9, 2)" in r.stdout
    assert "WRONG" not in r.stdout and "REFUSED" not in r.stdout


def test_new_symbols_declared_and_exported():
    L = _lib()
    names = kcnn.declared_symbols()
    for name in NEW:
        assert name in names, name
        assert hasattr(L, name), name


@pytest.fixture()
def net():
    L = _lib()
    h = L.kcnn_nnet_new(CONFIG)
    assert h, L.kcnn_last_error()
    yield ctypes.c_void_p(h)
    L.kcnn_nnet_free(ctypes.c_void_p(h))


def compute(fn, net, rows, cols, lengths, pad_input=1, priors=None, apply_log=0):
    L = _lib()
    lens = np.asarray(lengths, np.int32)
    data, d = ctypes.c_void_p(), kcnn.MatrixDim()
    pp, n = None, 0
    if priors is not None:
        pr = np.asarray(priors, np.float32)
        pp, n = pr.ctypes.data_as(ctypes.c_void_p), len(pr)
    rc = getattr(L, fn)(net, None, kcnn.MatrixDim(rows, cols, cols),
                        lens.ctypes.data_as(ctypes.c_void_p), len(lens), pad_input, pp, n,
                        ctypes.c_float(1.0), apply_log, ctypes.byref(data), ctypes.byref(d))
    return rc, L.kcnn_last_error().decode()


def refusals():
    good = np.full(90, 0.5, np.float32)
    cases = [
        (dict(rows=7, cols=5, lengths=[3, 3]), "sum to 6"),
        (dict(rows=7, cols=5, lengths=[0, 7]), "utterance 0 has 0"),
        (dict(rows=7, cols=5, lengths=[8, -1]), "utterance 1 has -1"),
        (dict(rows=7, cols=5, lengths=[]), "no utterances"),
        (dict(rows=11, cols=5, lengths=[11], pad_input=0), "at least 12"),
        (dict(rows=7, cols=4, lengths=[7]), "columns"),
        (dict(rows=7, cols=5, lengths=[7], priors=good[:89], apply_log=1), "89 priors for 90"),
        (dict(rows=7, cols=5, lengths=[7], priors=good, apply_log=0), "apply_log"),
    ]
    for bad in (0.0, -1.0, np.nan, np.inf):
        pr = good.copy()
        pr[9] = bad
        cases.append((dict(rows=7, cols=5, lengths=[7], priors=pr, apply_log=1), "prior 9"))
    return cases


@pytest.mark.parametrize("kw, what", refusals(), ids=[f"{i}-{w}" for i, (_, w) in
                                                       enumerate(refusals())])
def test_shared_refuses_what_compute_refuses(net, kw, what):
    rc0, msg0 = compute("kcnn_nnet_compute", net, **kw)
    rc1, msg1 = compute("kcnn_nnet_compute_shared", net, **kw)
    assert rc0 != 0 and what in msg0, (rc0, msg0)
    assert rc1 != 0 and what in msg1, (rc1, msg1)
    # the same message under the other name
    assert msg1.replace("kcnn_nnet_compute_shared", "kcnn_nnet_compute") == msg0


def test_shared_refuses_missing_result_pointers(net):
    L = _lib()
    lens = np.asarray([7], np.int32)
    rc = L.kcnn_nnet_compute_shared(net, None, kcnn.MatrixDim(7, 5, 5),
                                    lens.ctypes.data_as(ctypes.c_void_p), 1, 1, None, 0,
                                    ctypes.c_float(1.0), 0, None, None)
    assert rc != 0 and "no result pointers" in L.kcnn_last_error().decode()


def test_prefix_of_networks_the_plan_declines(net):
    """No device: two Splices (a context above component 0), a Softmax alone,
    a Splice with a const tail."""
    L = _lib()
    assert L.kcnn_nnet_time_shared_prefix(net) == 0
    for config in (b"SoftmaxComponent dim=12",
                   b"SpliceComponent input-dim=6 left-context=1 right-context=1 "
                   b"const-component-dim=2\nSoftmaxComponent dim=14",
                   b"SpliceComponent input-dim=4 left-context=2 right-context=2 "
                   b"const-component-dim=0\nRectifiedLinearComponent dim=20"):
        h = L.kcnn_nnet_new(config)
        assert h, L.kcnn_last_error()
        try:
            assert L.kcnn_nnet_time_shared_prefix(ctypes.c_void_p(h)) == 0
        finally:
            L.kcnn_nnet_free(ctypes.c_void_p(h))


def test_time_map_without_a_shared_pass_is_an_error_code(net):
    L = _lib()
    p, d = ctypes.c_void_p(), kcnn.MatrixDim()
    c, n, dil = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = L.kcnn_nnet_time_map(net, 0, ctypes.byref(p), ctypes.byref(d), ctypes.byref(c),
                              ctypes.byref(n), ctypes.byref(dil))
    assert rc != 0 and "kcnn_nnet_compute_shared" in L.kcnn_last_error().decode()
    rc = L.kcnn_nnet_time_map(net, 0, None, None, None, None, None)
    assert rc != 0 and "no result pointers" in L.kcnn_last_error().decode()
