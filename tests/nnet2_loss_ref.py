"""numpy restatement of SoftmaxComponent, DropoutComponent and the
cross-entropy objective (reference nnet2/nnet-component.cc:930-1000,
:3540-3643; cudamatrix/cu-matrix.h:624-637 CompObjfAndDeriv), written from
their definitions: fp32 forms in the reference's operation order, fp64 forms
as the truth the 1e-5 bars are taken against, and a Philox4x32-10 (Salmon et
al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) for the dropout
masks.
"""
import numpy as np

SOFTMAX_FLOOR = 1.0e-20
F32 = np.float32
# the seed the GPU tests give their DropoutComponents (test_nnet2_loss_ref.py
# checks the generator's draws under it on the CPU)
DROPOUT_SEED = 0x1234ABCD5678EF01

# ---- Philox4x32-10 ---------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words c0..c3 (arrays or ints, broadcast together) and key words
    k0, k1 (ints) -> the four uint32 output words."""
    c = [np.asarray(v, np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _MASK, p1 >> _S32, p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def dropout_uniform(seed, call, rows, cols):
    """The uniform draw of every element of a [rows x cols] matrix in
    Propagate call `call` of a component seeded `seed`: key = the 64-bit seed,
    counter = (col // 4, row, call low, call high), output word col % 4,
    u = (x >> 8) * 2^-24 (exact in fp32)."""
    ncb = (cols + 3) // 4
    cb, row = np.meshgrid(np.arange(ncb), np.arange(rows))
    out = philox4x32_10(cb, row, call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF,
                        seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    x = np.stack(out, axis=-1).reshape(rows, ncb * 4)[:, :cols]
    return (x >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


# ---- Dropout -----------------------------------------------------------------
def dropout_scales(dp, scale):
    """(low, high - low) as the reference computes them: the fp32 product
    dp * low, the rest in double, rounded to fp32 (BaseFloat high_scale); the
    difference in fp32."""
    dp, low = F32(dp), F32(scale)
    assert 0.0 <= dp < 1.0 and 0.0 <= low <= 1.0
    high = F32((1.0 - float(F32(dp * low))) / (1.0 - float(dp)))
    assert abs(float(low) * float(dp) + float(high) * (1.0 - float(dp)) - 1.0) < 0.01
    return low, F32(high - low)


def dropout_mask(u, dp, scale):
    """Add(-dp), ApplyHeaviside, Scale(high - low) unless 1, Add(low) unless 0;
    every step in fp32."""
    low, hl = dropout_scales(dp, scale)
    m = ((u - F32(dp)) > 0).astype(F32)
    if hl != 1.0:
        m = m * hl
    if low != 0.0:
        m = m + low
    return m.astype(F32)


def dropout_prop(x, dp, scale, seed, call):
    return dropout_mask(dropout_uniform(seed, call, *x.shape), dp, scale) * x.astype(F32)


def dropout_backprop(in_value, out_value, out_deriv):
    """AddMatMatDivMat: in_value == 0 ? out_deriv : out_deriv * out_value /
    in_value, the fp32 product first, then an IEEE divide."""
    with np.errstate(all="ignore"):
        q = (out_deriv.astype(F32) * out_value.astype(F32)).astype(F32) / in_value.astype(F32)
    return np.where(in_value == 0, out_deriv, q).astype(F32)


# ---- Softmax -------------------------------------------------------------------
def softmax_raw64(x):
    """Per row exp(x - max) / sum in fp64, before the floor."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        t = np.exp(x - x.max(axis=1, keepdims=True))
        return t / t.sum(axis=1, keepdims=True)


def softmax_prop64(x):
    """softmax_raw64, then ApplyFloor(1e-20) (NaN stays)."""
    y = softmax_raw64(x)
    with np.errstate(all="ignore"):
        return np.where(y < SOFTMAX_FLOOR, SOFTMAX_FLOOR, y)


def softmax_backprop64(p, e):
    """D = P o E - diag(rowdot(P, E)) P and the error scale sum_j |P_j E_j|."""
    p, e = np.asarray(p, np.float64), np.asarray(e, np.float64)
    pe = p * e
    return pe - pe.sum(axis=1, keepdims=True) * p, np.abs(pe).sum(axis=1, keepdims=True)


# ---- CompObjfAndDeriv -------------------------------------------------------------
def comp_objf_and_deriv32(probs, labels, deriv):
    """deriv(row, col) += weight / probs(row, col) in fp32; returns the new
    deriv, the fp64 sum of weight * log probs(row, col) and of weight."""
    d = np.array(deriv, F32)
    objf = tot = 0.0
    for r, c, w in labels:
        d[r, c] = d[r, c] + F32(w) / F32(probs[r, c])
        objf += float(F32(w)) * np.log(np.float64(probs[r, c]))
        tot += float(F32(w))
    return d, objf, tot


def xent_deriv64(p, labels):
    """The derivative into a final Softmax for labels on its output P:
    D[r, c] = [label c] w_c - P[r, c] S_r, S_r the row's weight; and S_r."""
    p = np.asarray(p, np.float64)
    w = np.zeros_like(p)
    for r, c, wt in labels:
        w[r, c] += float(F32(wt))
    s = w.sum(axis=1, keepdims=True)
    return w - p * s, s


# ---- FullyConnectedComponent in fp64 (reference nnet-component-nnet0.cc:1133-1150) ----
class FC64:
    """y = x W^T + b; the update prev = m prev - (lr / N) wd W + (lr / N) dY^T X,
    W += prev, b += (lr / N) colsum(dY)."""

    def __init__(self, W, b, prev, lr, wd, m):
        self.W, self.b, self.prev = (np.array(a, np.float64) for a in (W, b, prev))
        self.lr, self.wd, self.m = lr, wd, m

    def propagate(self, x):
        return x @ self.W.T + self.b

    def backprop(self, x, dy):
        dx = dy @ self.W
        lr = self.lr / x.shape[0]
        self.b = self.b + lr * dy.sum(axis=0)
        self.prev = self.m * self.prev - lr * self.wd * self.W + lr * (dy.T @ x)
        self.W = self.W + self.prev
        return dx
