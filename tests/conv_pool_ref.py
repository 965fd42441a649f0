"""Host definitions of the fused conv + pool entry points' pooled output, routing
mask and mask expansion (include/cnsl-hip-kernels.h), in numpy: selects and
comparisons only, no arithmetic.  tests/test_conv_pool_ref.py checks them
against the oracle's Maxpool (A.8 / A.9); tests/test_gpu_conv_pool.py checks the
kernels against them.

Y [R x G*P], column g*P + x*oh + y.  A ph x pw x pc window (c, w, h) of pooled
value (gj, wx, hy) is Y's map pc*gj + c at position (pw*wx + w, ph*hy + h);
the pooled column is (gj*(ow/pw) + wx)*(oh/ph) + hy and the window element's
mask bit c*pw*ph + w*ph + h.
"""
import numpy as np


def windows(Y, G, oh, ow, win):
    """[R, pooled columns, ph*pw*pc]: the window elements of every pooled
    value, in mask-bit order."""
    ph, pw, pc = win
    R = Y.shape[0]
    a = np.asarray(Y).reshape(R, G // pc, pc, ow // pw, pw, oh // ph, ph)
    a = a.transpose(0, 1, 3, 5, 2, 4, 6)
    return a.reshape(R, G // pc * (ow // pw) * (oh // ph), pc * pw * ph)


def unwindows(Wn, G, oh, ow, win):
    """The inverse of windows(): [R, G*P]."""
    ph, pw, pc = win
    R = Wn.shape[0]
    a = np.asarray(Wn).reshape(R, G // pc, ow // pw, oh // ph, pc, pw, ph)
    a = a.transpose(0, 1, 4, 2, 5, 3, 6)
    return np.ascontiguousarray(a).reshape(R, G * oh * ow)


def max_window(Y, G, oh, ow, win):
    return windows(Y, G, oh, ow, win).max(axis=2)


def mask_of(Y, pooled, G, oh, ow, win):
    """The header's mask: bit k = (window element k == pooled value)."""
    w = windows(Y, G, oh, ow, win)
    hit = (w == np.asarray(pooled)[:, :, None]).astype(np.uint32)
    return (hit << np.arange(w.shape[2], dtype=np.uint32)).sum(axis=2).astype(np.uint32)


def expand(mask, dP, G, oh, ow, win):
    """hipF_maxpool_backprop_mask[3d]: dY = dP of its window where the bit is set, else 0."""
    n = win[0] * win[1] * win[2]
    bit = (np.asarray(mask, np.uint32)[:, :, None] >> np.arange(n, dtype=np.uint32)) & 1
    w = np.where(bit != 0, np.asarray(dP, np.float32)[:, :, None], np.float32(0))
    return unwindows(w.astype(np.float32), G, oh, ow, win)


def window_bits(win):
    return (1 << (win[0] * win[1] * win[2])) - 1
