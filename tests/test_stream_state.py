"""The streaming forward pass, without a GPU: the host bookkeeping of
kcnn::OnlineComputer (capi/stream-state.h) run as a stand-alone program under
AddressSanitizer and UBSan, and the kcnn_online_* entry points' refusals,
which answer with an error code and a message before any device is touched:
the arena is allocated by the first accepted step, the networks below own no
device memory, and a refused call launches nothing and moves no slot."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import kcnn
from test_abi import _lib
from test_frame_index import CONFIG, WIDE, nnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kcnn_online_new", "kcnn_online_free", "kcnn_online_accept", "kcnn_online_reset",
       "kcnn_online_frames")
STREAMS, MAX_CHUNK = 4, 6


def test_stream_state_program_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "stream_state_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src"),
                    os.path.join(ROOT, "scripts", "stream_state_check.cc"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all stream state checks passed" in r.stdout
    assert "WRONG" not in r.stdout and "REFUSED" not in r.stdout


def test_new_symbols_declared_and_exported():
    L = _lib()
    names = kcnn.declared_symbols()
    for name in NEW:
        assert name in names, name
        assert hasattr(L, name), name


def online_new(net, num_streams=STREAMS, max_chunk=MAX_CHUNK, priors=None, num_priors=None,
               apply_log=False):
    """(handle or None, message)"""
    L = _lib()
    pp, n = None, 0
    if priors is not None:
        pr = np.asarray(priors, np.float32)
        pp, n = pr.ctypes.data_as(ctypes.c_void_p), len(pr)
    h = L.kcnn_online_new(net, num_streams, max_chunk, pp, n if num_priors is None else num_priors,
                          ctypes.c_float(1.0), int(apply_log))
    return (ctypes.c_void_p(h) if h else None), L.kcnn_last_error().decode()


def all_frames(o, num_streams=STREAMS):
    L = _lib()
    out = []
    for s in range(num_streams):
        f = (ctypes.c_int64 * 2)(-1, -1)
        assert L.kcnn_online_frames(o, s, f) == 0, L.kcnn_last_error()
        out.append((f[0], f[1]))
    return out


def accept(o, streams, num_new, final, rows=None, cols=5, stride=None, chunk=True):
    """(rc, message, num_out); the chunk pointer is never read on the host."""
    L = _lib()
    st, nn, fi = (np.asarray(a, np.int32) for a in (streams, num_new, final))
    fake = np.zeros(4, np.float32)  # stands for the device matrix
    rows = int(sum(num_new)) if rows is None else rows
    counts = np.full(len(st) + 1, -5, np.int32)
    p, od = ctypes.c_void_p(), kcnn.MatrixDim()
    rc = L.kcnn_online_accept(
        o, fake.ctypes.data_as(ctypes.c_void_p) if chunk else None,
        kcnn.MatrixDim(rows, cols, cols if stride is None else stride),
        st.ctypes.data_as(ctypes.c_void_p), nn.ctypes.data_as(ctypes.c_void_p),
        fi.ctypes.data_as(ctypes.c_void_p), len(st), counts.ctypes.data_as(ctypes.c_void_p),
        ctypes.byref(p), ctypes.byref(od))
    return rc, L.kcnn_last_error().decode(), counts


@pytest.fixture()
def net():
    h = nnet(CONFIG)
    yield h
    _lib().kcnn_nnet_free(h)


def test_new_refusals(net):
    L = _lib()
    good = np.full(30, 0.25, np.float32)
    for kw, what in (
            ({"num_streams": 0}, "num_streams 0"),
            ({"num_streams": -3}, "num_streams -3"),
            ({"max_chunk": 0}, "max_chunk 0"),
            ({"max_chunk": -1}, "max_chunk -1"),
            ({"num_streams": 1 << 26, "max_chunk": 11}, "2^31"),  # 2 x 2^26 x 16 rows
            ({"num_streams": 1 << 22, "max_chunk": 59}, "2^31"),  # 2^29 rows of 5 columns
            ({"priors": good, "apply_log": False}, "priors without apply_log"),
            ({"priors": good[:29], "apply_log": True}, "29 priors for 30"),
            ({"priors": good, "num_priors": 31, "apply_log": True}, "31 priors for 30"),
    ):
        h, msg = online_new(net, **kw)
        assert h is None and what in msg, (kw, msg)
    for bad in (0.0, -0.5, np.nan, np.inf):
        pr = good.copy()
        pr[7] = bad
        h, msg = online_new(net, priors=pr, apply_log=True)
        assert h is None and "prior 7 is" in msg, (bad, msg)
    h, msg = online_new(None)
    assert h is None and "no network" in msg, msg
    # and the valid ones: no device is touched
    for kw in ({}, {"priors": good, "apply_log": True}, {"apply_log": True},
               {"num_streams": 1, "max_chunk": 1}):
        h, msg = online_new(net, **kw)
        assert h, msg
        assert all_frames(h, kw.get("num_streams", STREAMS)) == \
            [(0, 0)] * kw.get("num_streams", STREAMS)
        L.kcnn_online_free(h)


@pytest.fixture()
def online(net):
    h, msg = online_new(net)
    assert h, msg
    yield h
    _lib().kcnn_online_free(h)


REFUSED_STEPS = [
    (dict(streams=[0, 4], num_new=[1, 1], final=[0, 0]), "entry 1: stream 4 outside [0, 4)"),
    (dict(streams=[-1], num_new=[1], final=[0]), "entry 0: stream -1 outside"),
    (dict(streams=[2, 1, 2], num_new=[1, 1, 1], final=[0, 0, 1]), "stream 2 is named twice"),
    (dict(streams=[0, 1, 2, 3, 0], num_new=[1] * 5, final=[0] * 5), "5 slots named"),
    (dict(streams=[1], num_new=[-1], final=[1], rows=0), "-1 new frames outside [0, max_chunk = 6]"),
    (dict(streams=[1], num_new=[7], final=[0]), "7 new frames outside [0, max_chunk = 6]"),
    (dict(streams=[0, 1], num_new=[2, 0], final=[0, 0]), "entry 1: no new frames for stream 1"),
    (dict(streams=[0, 1], num_new=[2, 3], final=[0, 1], rows=6), "sum to 5, the chunk has 6 rows"),
    (dict(streams=[0, 1], num_new=[2, 3], final=[0, 1], rows=4), "sum to 5, the chunk has 4 rows"),
    (dict(streams=[0], num_new=[0], final=[1], rows=-1), "a chunk of -1 rows"),
    (dict(streams=[0], num_new=[2], final=[0], cols=4), "a chunk of 4 columns for a network of 5"),
    (dict(streams=[0], num_new=[2], final=[0], cols=6), "a chunk of 6 columns for a network of 5"),
    (dict(streams=[0], num_new=[2], final=[0], stride=4), "a row stride of 4 for 5 columns"),
    (dict(streams=[0], num_new=[2], final=[0], chunk=False), "no chunk"),
]


@pytest.mark.parametrize("kw, what", REFUSED_STEPS, ids=[w for _, w in REFUSED_STEPS])
def test_accept_refusals(online, kw, what):
    rc, msg, counts = accept(online, **kw)
    assert rc != 0 and what in msg, (rc, msg)
    assert (counts == -5).all(), "num_out was written by a refused step"
    assert all_frames(online) == [(0, 0)] * STREAMS


def test_accept_refuses_missing_arrays_and_handles(online):
    L = _lib()
    p, od = ctypes.c_void_p(), kcnn.MatrixDim()
    one = np.ones(1, np.int32)
    ip = one.ctypes.data_as(ctypes.c_void_p)
    d = kcnn.MatrixDim(1, 5, 5)
    assert L.kcnn_online_accept(online, ip, d, None, ip, ip, 1, ip, ctypes.byref(p),
                                ctypes.byref(od)) != 0
    assert "bad stream arrays" in L.kcnn_last_error().decode()
    assert L.kcnn_online_accept(online, ip, d, ip, ip, ip, 1, None, ctypes.byref(p),
                                ctypes.byref(od)) != 0
    assert "no num_out" in L.kcnn_last_error().decode()
    assert L.kcnn_online_accept(online, ip, d, ip, ip, ip, 1, ip, None, None) != 0
    assert "no result pointers" in L.kcnn_last_error().decode()
    assert L.kcnn_online_accept(None, ip, d, ip, ip, ip, 1, ip, ctypes.byref(p),
                                ctypes.byref(od)) != 0
    assert "no computer" in L.kcnn_last_error().decode()
    f = (ctypes.c_int64 * 2)()
    for s in (-1, STREAMS):
        assert L.kcnn_online_frames(online, s, f) != 0
        assert f"stream {s} outside [0, {STREAMS})" in L.kcnn_last_error().decode()
        assert L.kcnn_online_reset(online, s) != 0
        assert f"stream {s} outside [0, {STREAMS})" in L.kcnn_last_error().decode()
    assert L.kcnn_online_reset(online, 2) == 0
    assert all_frames(online) == [(0, 0)] * STREAMS


def test_a_step_that_names_no_slot_runs_nothing(online):
    rc, msg, counts = accept(online, [], [], [], chunk=False)
    assert rc == 0, msg
    assert all_frames(online) == [(0, 0)] * STREAMS


def test_activations_reaching_2_31_are_an_error_code():
    """A window of 2 000 001 input rows an example: a final step that emits
    1100 frames asks for 2^31 rows of it, one that emits 1073 for 2^31
    elements.  Refused before the arena is asked for."""
    L = _lib()
    wide = nnet(WIDE)
    h, msg = online_new(wide, num_streams=2, max_chunk=1100)
    assert h, msg
    try:
        for n in (1100, 1073):
            rc, msg, _ = accept(h, [1], [n], [1], cols=4)
            assert rc != 0 and "2^31 rows or elements" in msg, (rc, msg)
            assert all_frames(h, 2) == [(0, 0)] * 2
    finally:
        L.kcnn_online_free(h)
        L.kcnn_nnet_free(wide)
