"""The whole-utterance forward's C entry points without a GPU: declared,
exported, and their host-side checks answer with an error code and a message
before any device is touched (neither network below owns device memory)."""
import ctypes

import numpy as np
import pytest

import kcnn
from test_abi import _lib

NEW = ("kcnn_nnet_left_context", "kcnn_nnet_right_context", "kcnn_nnet_compute")
CONFIG = (b"SpliceComponent input-dim=5 left-context=2 right-context=3 const-component-dim=0\n"
          b"SpliceComponent input-dim=30 context=-3:0:3 const-component-dim=0\n"
          b"SoftmaxComponent dim=90")


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


def test_contexts_are_the_sums_over_the_components(net):
    L = _lib()
    assert L.kcnn_nnet_left_context(net) == 5
    assert L.kcnn_nnet_right_context(net) == 6


def compute(net, rows, cols, lengths, pad_input=1, priors=None, apply_log=0):
    L = _lib()
    lens = np.asarray(lengths, np.int32)
    data, d = ctypes.c_void_p(), kcnn.MatrixDim()
    pp, n = None, 0
    if priors is not None:
        pr = np.asarray(priors, np.float32)
        pp, n = pr.ctypes.data_as(ctypes.c_void_p), len(pr)
    rc = L.kcnn_nnet_compute(net, None, kcnn.MatrixDim(rows, cols, cols),
                             lens.ctypes.data_as(ctypes.c_void_p), len(lens), pad_input, pp, n,
                             ctypes.c_float(1.0), apply_log, ctypes.byref(data), ctypes.byref(d))
    return rc, L.kcnn_last_error().decode()


@pytest.mark.parametrize("lengths, what", [
    ([3, 3], "sum to 6"),          # sum != rows
    ([0, 7], "utterance 0 has 0"),
    ([8, -1], "utterance 1 has -1"),
    ([], "no utterances"),
])
def test_bad_lengths_are_an_error_code(net, lengths, what):
    rc, msg = compute(net, 7, 5, lengths)
    assert rc != 0 and what in msg, (rc, msg)


def test_unpadded_needs_more_than_the_context(net):
    rc, msg = compute(net, 11, 5, [11], pad_input=0)  # T = L + R
    assert rc != 0 and "at least 12" in msg, (rc, msg)


def test_wrong_columns_and_bad_priors_are_an_error_code(net):
    rc, msg = compute(net, 7, 4, [7])
    assert rc != 0 and "columns" in msg, (rc, msg)
    good = np.full(90, 0.5, np.float32)
    for bad in (0.0, -1.0, np.nan, np.inf):
        pr = good.copy()
        pr[9] = bad
        rc, msg = compute(net, 7, 5, [7], priors=pr, apply_log=1)
        assert rc != 0 and "prior 9" in msg, (rc, msg)
    rc, msg = compute(net, 7, 5, [7], priors=good[:89], apply_log=1)
    assert rc != 0 and "89 priors for 90" in msg, (rc, msg)
    rc, msg = compute(net, 7, 5, [7], priors=good, apply_log=0)
    assert rc != 0 and "apply_log" in msg, (rc, msg)
