"""numpy fp64 restatement of NormalizeComponent (reference
nnet2/nnet-component.cc:576-639, nnet-component.h:555-582).

Per row of D columns: p = mean(x^2), floored at kNormFloor = 2^-66;
f = p^-0.5 (2^33 on the floor); out = x f.  Backprop: in_deriv = f dy -
(g / D) (sum dy x) x with g = f^3, or 0 where p <= kNormFloor (the reference's
ReplaceValue(2^33, 0): a row exactly on the floor counts as floored)."""
import numpy as np

NORM_FLOOR = 2.0 ** -66


def mean_square64(x):
    x = np.asarray(x, np.float64)
    return (x * x).sum(axis=1) / x.shape[1]


def scale64(x):
    """(f, g) per row, as columns."""
    p = mean_square64(x)
    f = np.maximum(p, NORM_FLOOR) ** -0.5
    g = np.where(p <= NORM_FLOOR, 0.0, f ** 3)
    return f[:, None], g[:, None]


def prop64(x):
    x = np.asarray(x, np.float64)
    f, _ = scale64(x)
    return x * f


def backprop64(x, dy):
    """(in_deriv, per-element sum of |terms|): |f dy_j| + (g / D) (sum_k
    |dy_k x_k|) |x_j|, the error scale of the two-term sum."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    D = x.shape[1]
    f, g = scale64(x)
    dot = (dy * x).sum(axis=1, keepdims=True)
    adot = np.abs(dy * x).sum(axis=1, keepdims=True)
    value = f * dy - (g / D) * dot * x
    terms = np.abs(f * dy) + (g / D) * adot * np.abs(x)
    return value, terms
