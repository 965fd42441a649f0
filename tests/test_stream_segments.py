"""The time-shared streaming step, without a GPU: its host plan
(StreamState::Segments of capi/stream-state.h with the row plan of
capi/time-plan.h) run as a stand-alone program under AddressSanitizer and
UBSan, and the new kcnn_online_* entry points, which touch no device: a
computer is made and asked for its prefix on networks that own no device
memory."""
import ctypes
import os
import shutil
import subprocess

import kcnn
from test_abi import _lib
from test_frame_index import CONFIG, nnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kcnn_online_new_shared", "kcnn_online_shared_prefix")


def test_stream_segments_program_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "stream_segments_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src"),
                    os.path.join(ROOT, "scripts", "stream_segments_check.cc"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all stream segment checks passed" in r.stdout
    assert "WRONG" not in r.stdout and "REFUSED" not in r.stdout


def test_new_symbols_declared_and_exported():
    L = _lib()
    names = kcnn.declared_symbols()
    for name in NEW:
        assert name in names, name
        assert hasattr(L, name), name


def new_shared(net, share_time, num_streams=4, max_chunk=6):
    L = _lib()
    L.kcnn_online_new_shared.restype = ctypes.c_void_p
    L.kcnn_online_new_shared.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                         ctypes.c_int, ctypes.c_int]
    L.kcnn_online_shared_prefix.argtypes = [ctypes.c_void_p]
    h = L.kcnn_online_new_shared(net, num_streams, max_chunk, None, 0, ctypes.c_float(1.0), 0,
                                 int(share_time))
    return (ctypes.c_void_p(h) if h else None), L.kcnn_last_error().decode()


def test_shared_prefix_without_a_device():
    """A network without a Convolution has no prefix, with share_time or
    without; the prefixes above 0 are tests/test_gpu_online_shared.py's."""
    L = _lib()
    net = nnet(CONFIG)
    shared, _ = new_shared(net, True)
    plain, _ = new_shared(net, False)
    assert shared and plain
    try:
        assert L.kcnn_nnet_time_shared_prefix(net) == 0
        assert L.kcnn_online_shared_prefix(shared) == 0
        assert L.kcnn_online_shared_prefix(plain) == 0
        assert L.kcnn_online_shared_prefix(None) == -1
        assert "no computer" in L.kcnn_last_error().decode()
        f = (ctypes.c_int64 * 2)(-1, -1)
        assert L.kcnn_online_frames(shared, 3, f) == 0 and tuple(f) == (0, 0)
    finally:
        L.kcnn_online_free(shared)
        L.kcnn_online_free(plain)
        L.kcnn_nnet_free(net)


def test_new_shared_refuses_what_new_refuses():
    net = nnet(CONFIG)
    try:
        for kw, what in (({"num_streams": 0}, "num_streams 0"), ({"max_chunk": 0}, "max_chunk 0")):
            o, msg = new_shared(net, True, **kw)
            assert o is None and what in msg, msg
        o, msg = new_shared(None, True)
        assert o is None and "no network" in msg
    finally:
        _lib().kcnn_nnet_free(net)
