"""conv_pool_ref.py's window layout, mask and mask expansion against the
oracle's MaxpoolComponent (A.8 Propagate, A.9 Backprop): the GPU tests of the
fused conv + pool entry points stand on these definitions."""
import numpy as np
import pytest

import conv_pool_ref as PR
import oracle as O
from _util import randn, rng, with_ties

WINDOWS = [(6, 4, 8, (1, 1, 4)), (6, 4, 8, (1, 1, 8)), (6, 4, 8, (2, 1, 4)), (6, 4, 4, (3, 1, 4)),
           (6, 4, 4, (1, 2, 1)), (6, 4, 4, (2, 2, 2)), (6, 4, 6, (3, 2, 2)), (1, 6, 4, (1, 2, 4))]


@pytest.mark.parametrize("oh,ow,G,win", WINDOWS)
@pytest.mark.parametrize("ties", [False, True])
def test_pool_mask_expand_match_the_oracle(oh, ow, G, win, ties):
    r = rng(oh + 10 * G + sum(win))
    ph, pw, pc = win
    Y = (with_ties if ties else randn)(r, (5, G * oh * ow))
    ncol = G * oh * ow // (ph * pw * pc)
    pooled = O.maxpool_prop(Y, oh, ow, ph, pw, pc, ncol)
    assert (PR.max_window(Y, G, oh, ow, win) == pooled).all()
    mask = PR.mask_of(Y, pooled, G, oh, ow, win)
    assert mask.min() >= 1 and mask.max() <= PR.window_bits(win)
    assert ties == bool((mask & (mask - 1)).any())       # a tie sets two bits
    dP = randn(r, (5, ncol))
    want = O.maxpool_backprop(Y, pooled, dP, oh, ow, ph, pw, pc)
    assert (PR.expand(mask, dP, G, oh, ow, win) == want).all()
    assert (PR.unwindows(PR.windows(Y, G, oh, ow, win), G, oh, ow, win) == Y).all()
