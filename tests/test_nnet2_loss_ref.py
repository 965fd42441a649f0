"""CPU checks behind tests/test_gpu_nnet2_loss.py: the numpy Philox4x32-10
of nnet2_loss_ref.py against the published known answer, the dropout test's
seed, and the Dropout / Softmax model fixtures against their encoder."""
import os

import numpy as np
import pytest

import kaldi_binary_nnet2 as KB2
import nnet2_loss_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = os.path.join(GOLDEN, "models")
DROPOUT_SEED = R.DROPOUT_SEED


def test_philox_known_answer():
    # Random123 kat_vectors: philox4x32-10, zero counter, zero key
    out = R.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # and the all-ones / pi-digits vectors of the same file
    out = R.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    out = R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(v) for v in out] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_philox_broadcasts_like_the_scalar_form():
    cb, row = np.meshgrid(np.arange(5), np.arange(3))
    out = R.philox4x32_10(cb, row, 7, 0, 11, 13)
    one = R.philox4x32_10(4, 2, 7, 0, 11, 13)
    assert [int(o[2, 4]) for o in out] == [int(v) for v in one]


def test_dropout_seed_share_and_no_zero_draw():
    """A deterministic statement about the generator with the GPU test's
    seed: over 70 x 4096 draws at dp = 0.5 the dropped share is within 5
    sigma of 0.5 (binomial sigma = 268 of 286,720: +-0.0047), and no draw of
    the calls the GPU test makes is exactly 0 (with dp = 0 a zero draw is the
    one element Heaviside(u - 0) drops, and the test expects the identity)."""
    n = 70 * 4096
    for call in range(3):
        u = R.dropout_uniform(DROPOUT_SEED, call, 70, 4096)
        assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
        dropped = float((R.dropout_mask(u, 0.5, 0.0) == 0).sum()) / n
        assert abs(dropped - 0.5) <= 5 * np.sqrt(n * 0.25) / n, dropped
        assert (u > 0).all()
        assert (R.dropout_uniform(DROPOUT_SEED, call, 70, 4095) > 0).all()
    # the mask depends on the element's position alone: a narrower matrix is
    # the same draws
    np.testing.assert_array_equal(R.dropout_uniform(DROPOUT_SEED, 1, 70, 4095),
                                  R.dropout_uniform(DROPOUT_SEED, 1, 70, 4096)[:, :4095])


def test_dropout_scales():
    assert R.dropout_scales(0.5, 0.0) == (0.0, 2.0)
    assert R.dropout_scales(0.5, 1.0) == (1.0, 0.0)
    assert R.dropout_scales(0.0, 0.0) == (0.0, 1.0)
    low, hl = R.dropout_scales(0.2, 0.5)
    assert low == 0.5 and abs(float(hl) - 0.625) < 1e-6


def _params(kind):
    z = np.load(os.path.join(MODELS, f"{kind}.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("kind", ["dropout", "softmax"])
def test_fixture_matches_spec_encoder(kind):
    data = open(os.path.join(MODELS, f"{kind}.bin"), "rb").read()
    assert data == KB2.encode(kind, _params(kind))
    assert data.startswith(b"\x00B<")


def test_dropout_token_order_is_scale_then_proportion():
    data = open(os.path.join(MODELS, "dropout.bin"), "rb").read()
    assert 0 < data.index(b"<DropoutScale>") < data.index(b"<DropoutProportion>")


def test_reference_settings_files():
    lines = [l for l in open(os.path.join(GOLDEN, "nnet.config")).read().splitlines() if l.strip()]
    assert len(lines) == 22
    assert lines[16].split()[0] == lines[19].split()[0] == "DropoutComponent"
    assert lines[21] == "SoftmaxComponent dim=3454"
    scales = open(os.path.join(GOLDEN, "dropout_scale.config")).read().strip().split(":")
    assert [float(s) for s in scales] == [1, 1, 1, 1, 1, 1, 0.5, 0.5, 1]
