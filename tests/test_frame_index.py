"""Training from a device-resident corpus, without a GPU: the host routine
that checks and stages a minibatch of corpus rows (capi/frame-index.h) run as
a stand-alone program under AddressSanitizer and UBSan, and the new C entry
points' refusals, which answer with an error code and a message before any
device is touched (the networks below own no device memory, and a refused
call launches nothing)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import kcnn
from test_abi import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kcnn_corpus_new", "kcnn_corpus_free", "kcnn_nnet_propagate_frames",
       "kcnn_nnet_compute_prob_frames")
CONFIG = (b"SpliceComponent input-dim=5 left-context=2 right-context=3 const-component-dim=0\n"
          b"SoftmaxComponent dim=30")
# a window of 2 000 001 input rows an example: 1100 examples reach 2^31 rows
WIDE = b"SpliceComponent input-dim=4 context=-1000000:0:1000000 const-component-dim=0"


def test_frame_index_program_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "frame_index_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src"),
                    os.path.join(ROOT, "scripts", "frame_index_check.cc"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all frame index checks passed" in r.stdout
    assert "WRONG" not in r.stdout and "REFUSED" not in r.stdout


def test_new_symbols_declared_and_exported():
    L = _lib()
    names = kcnn.declared_symbols()
    for name in NEW:
        assert name in names, name
        assert hasattr(L, name), name


def corpus_new(rows, cols, lengths, feats=True, stride=None):
    """(handle or None, message); the feature pointer is never read on the host."""
    L = _lib()
    lens = np.asarray(lengths, np.int32)
    fake = np.zeros(4, np.float32)  # stands for the device matrix
    h = L.kcnn_corpus_new(fake.ctypes.data_as(ctypes.c_void_p) if feats else None,
                          kcnn.MatrixDim(rows, cols, cols if stride is None else stride),
                          lens.ctypes.data_as(ctypes.c_void_p), len(lens))
    return (ctypes.c_void_p(h) if h else None), L.kcnn_last_error().decode()


@pytest.mark.parametrize("lengths, what", [
    ([3, 3], "sum to 6"),
    ([4, 4], "sum to 8"),
    ([0, 7], "utterance 0 has 0"),
    ([8, -1], "utterance 1 has -1"),
    ([], "no utterances"),
])
def test_corpus_refuses_bad_lengths(lengths, what):
    h, msg = corpus_new(7, 5, lengths)
    assert h is None and what in msg, msg


def test_corpus_refuses_bad_matrices():
    for args, what in (((0, 5, []), "no utterances"), ((0, 5, [1]), "empty"),
                       ((1 << 26, 32, [1 << 26]), "2^31")):
        h, msg = corpus_new(*args)
        assert h is None and what in msg, msg
    h, msg = corpus_new(7, 5, [7], feats=False)
    assert h is None and "no feature matrix" in msg, msg
    h, msg = corpus_new(7, 5, [7], stride=4)
    assert h is None and "stride" in msg, msg


@pytest.fixture()
def corpus():
    h, msg = corpus_new(12, 5, [1, 7, 4])
    assert h, msg
    yield h
    _lib().kcnn_corpus_free(h)


def nnet(config):
    L = _lib()
    h = L.kcnn_nnet_new(config)
    assert h, L.kcnn_last_error()
    return ctypes.c_void_p(h)


def propagate_frames(net, corpus, frames):
    L = _lib()
    fr = np.asarray(frames, np.int32)
    rc = L.kcnn_nnet_propagate_frames(net, corpus, fr.ctypes.data_as(ctypes.c_void_p), len(fr))
    return rc, L.kcnn_last_error().decode()


def test_propagate_frames_refusals_are_an_error_code(corpus):
    L = _lib()
    net = nnet(CONFIG)
    try:
        for frames, what in (([], "no frames"), ([0, 12], "frame 1: row 12 outside [0, 12)"),
                             ([-1], "frame 0: row -1"), ([3, 11, -2147483648], "frame 2")):
            rc, msg = propagate_frames(net, corpus, frames)
            assert rc != 0 and what in msg, (rc, msg)
        rc, msg = propagate_frames(net, None, [0])
        assert rc != 0 and "no corpus" in msg, (rc, msg)
        # the labels' checks follow the frames'
        fr = np.asarray([0, 5], np.int32)
        rows, cols = np.asarray([0, 2], np.int32), np.asarray([1, 1], np.int32)
        w = np.ones(2, np.float32)
        rc = L.kcnn_nnet_compute_prob_frames(
            net, corpus, fr.ctypes.data_as(ctypes.c_void_p), 2,
            rows.ctypes.data_as(ctypes.c_void_p), cols.ctypes.data_as(ctypes.c_void_p),
            w.ctypes.data_as(ctypes.c_void_p), 2)
        assert rc != 0 and "row 2 outside [0, 2)" in L.kcnn_last_error().decode()
        rc = L.kcnn_nnet_compute_prob_frames(
            net, corpus, fr.ctypes.data_as(ctypes.c_void_p), 0,
            rows.ctypes.data_as(ctypes.c_void_p), cols.ctypes.data_as(ctypes.c_void_p),
            w.ctypes.data_as(ctypes.c_void_p), 2)
        assert rc != 0 and "no frames" in L.kcnn_last_error().decode()
    finally:
        L.kcnn_nnet_free(net)


def test_wrong_columns_are_an_error_code():
    L = _lib()
    net = nnet(CONFIG)
    h, msg = corpus_new(12, 4, [12])
    assert h, msg
    try:
        rc, msg = propagate_frames(net, h, [0])
        assert rc != 0 and "4 columns for a network of 5" in msg, (rc, msg)
    finally:
        L.kcnn_corpus_free(h)
        L.kcnn_nnet_free(net)


def test_window_rows_reaching_2_31_are_an_error_code():
    L = _lib()
    net = nnet(WIDE)
    assert L.kcnn_nnet_left_context(net) == 1000000
    h, msg = corpus_new(12, 4, [12])
    assert h, msg
    try:
        rc, msg = propagate_frames(net, h, [3] * 1100)  # 1100 x 2 000 001 rows
        assert rc != 0 and "2^31 rows" in msg, (rc, msg)
        # under 2^31 rows, but 1073 x 2 000 001 x 4 input elements
        rc, msg = propagate_frames(net, h, [3] * 1073)
        assert rc != 0 and "2^31 rows or elements" in msg, (rc, msg)
    finally:
        L.kcnn_corpus_free(h)
        L.kcnn_nnet_free(net)
