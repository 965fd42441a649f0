"""Pitched device matrices with sentinels, for the tests that call a kernel
launcher directly (kl_* in test_gpu_matrix_ops.py, kn_* in the nnet2 kernel
tests): what a kernel must not touch -- the floats before the base, the pad
columns of every row and a guard after the last row -- holds PAD, and
Mat.get() asserts that it still does.  Comparisons are bit for bit."""
import numpy as np

PAD = np.float32(-12345.5)
GUARD = 64


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


class Mat:
    """A pitched device matrix holding x; padding and guard hold PAD.

    stride = cols + extra unless given; `lead` floats of PAD come before the
    base (the allocation is at least 256-byte aligned, so lead = 1 makes a base
    that is only 4-byte aligned); `guard` floats of PAD follow the last row."""

    def __init__(self, kc, x, extra=3, lead=0, guard=GUARD, stride=None):
        import torch
        x = np.asarray(x, np.float32)
        if x.ndim == 1:
            x = x[None, :]
        self.rows, self.cols = x.shape
        self.stride = self.cols + extra if stride is None else stride
        assert self.stride >= self.cols and lead >= 0 and guard >= 0
        self.lead, self.guard = lead, guard
        self.h = np.full(lead + self.rows * self.stride + guard, PAD, np.float32)
        self.body()[:, :self.cols] = x
        self.t = torch.from_numpy(self.h.copy()).cuda()
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + 4 * lead
        self.dim = kc.MatrixDim(self.rows, self.cols, self.stride)

    def body(self, h=None):
        h = self.h if h is None else h
        return h[self.lead:self.lead + self.rows * self.stride].reshape(self.rows, self.stride)

    def get(self):
        """The matrix now; the lead, the padding and the guard must be as they were."""
        g = self.t.cpu().numpy()
        assert (g[:self.lead] == PAD).all(), "the floats before the base were written"
        assert (self.body(g)[:, self.cols:] == PAD).all(), "padding was written"
        assert (g[self.lead + self.rows * self.stride:] == PAD).all(), "guard was written"
        return self.body(g)[:, :self.cols].copy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(np.asarray(want, np.float32)))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[:3].tolist()}"


def place(kc, op, x=None):
    """A Mat laid out as the table's operand `op` (rows, cols, stride, lead)
    holding x, or NaN for an output; the guard is at least a row long."""
    rows, cols, stride, lead = op
    if x is None:
        x = np.full((rows, cols), np.nan)
    assert np.shape(x) == (rows, cols)
    return Mat(kc, x, stride=stride, lead=lead, guard=max(GUARD, cols))


def edge_columns(cols):
    """The last column, the last column of the last whole 4-column vector and
    the first column of the element-wise tail behind it (load_row / store_row
    of row-regs.h take the columns past cols // V * V one by one)."""
    whole = cols // 4 * 4
    return sorted({cols - 1, max(whole - 1, 0), min(whole, cols - 1)})
