"""kcnn -- Python host binding of libkcnn.so (the MI355X build of kaldi-cnn's
nnet2 CNN hot path).

Mirrors the reference's interfaces with the same names and argument meaning:

  * ``Mat*`` functions  = ``CuMatrixBase<float>::{Conv2D, AddMatRepVec,
    FlipMat, PaddingZero, TpBlock, TpInsideBlock, ModPermuteRow,
    Maxpool_prop, Maxpool_backprop}`` (reference cudamatrix/cu-matrix.h:451-480)
  * ``Component``       = nnet2 ``Component`` / ``UpdatableComponent`` as the
    nnet0 components implement them (nnet0/nnet-component-nnet0.h:23-232),
    created with ``Component.NewFromString`` (nnet2/nnet-component.cc:124-136)
  * ``Nnet``            = a component stack run NnetUpdater-style.
  * ``Corpus`` / ``train_epoch`` = training minibatches as rows of a corpus
    that stays on the device (nnet-get-egs + nnet-shuffle-egs + nnet-train).
  * ``OnlineComputer``  = upstream ``NnetOnlineComputer`` (the decodable of
    online2-wav-nnet2-latgen-faster) over concurrent utterances.

Matrices are 2-D float32 CUDA tensors with unit column stride (any row
stride); they are handed to the C++ library as raw device pointers + MatrixDim
on torch's current stream.  PyTorch is plumbing here (device memory, streams,
torch.distributed); every computation runs in libkcnn.so's HIP kernels.  There
is no fallback: if the library or a GPU is missing, calls raise.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KCNN_LIB: an alternative build of the same library (e.g. the phase-timing
# build, `make -C kaldi-cnn_amd timing`)
LIB_PATH = os.environ.get("KCNN_LIB") or os.path.join(_HERE, "libkcnn.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")


class KcnnError(RuntimeError):
    """A KALDI_ASSERT / KALDI_ERR / HIP error raised inside libkcnn.so."""


class MatrixDim(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("stride", ctypes.c_int32)]

    def __repr__(self):
        return f"MatrixDim({self.rows}, {self.cols}, {self.stride})"


_lib = None


def lib():
    """The loaded libkcnn.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: torch bundles libamdhip64.so.7 (same
        # SONAME as /opt/rocm's); loading torch first makes libkcnn.so bind
        # to that already-loaded runtime instead of a second copy.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise KcnnError(f"{LIB_PATH} not built (run `make -C kaldi-cnn_amd` "
                            "or __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        L.kcnn_last_error.restype = ctypes.c_char_p
        L.kcnn_version.restype = ctypes.c_char_p
        if hasattr(L, "kcnn_device_malloc_calls"):  # (absent from pre-r05 builds)
            L.kcnn_device_malloc_calls.restype = ctypes.c_ulonglong
        for name in ("kcnn_component_new_from_string", "kcnn_component_read",
                     "kcnn_component_copy"):
            getattr(L, name).restype = ctypes.c_void_p
        L.kcnn_component_new_from_string.argtypes = [ctypes.c_char_p]
        L.kcnn_component_read.argtypes = [ctypes.c_char_p]
        L.kcnn_component_copy.argtypes = [ctypes.c_void_p]
        L.kcnn_component_free.argtypes = [ctypes.c_void_p]
        L.kcnn_component_learning_rate.restype = ctypes.c_float
        L.kcnn_nnet_new.restype = ctypes.c_void_p
        L.kcnn_nnet_new.argtypes = [ctypes.c_char_p]
        if hasattr(L, "kcnn_nnet_read"):  # (absent from builds before the <Nnet> files)
            L.kcnn_nnet_read.restype = ctypes.c_void_p
            L.kcnn_nnet_read.argtypes = [ctypes.c_char_p]
            L.kcnn_nnet_write.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
            L.kcnn_nnet_copy.restype = ctypes.c_void_p
            L.kcnn_nnet_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_int]
        if hasattr(L, "kcnn_corpus_new"):  # (absent from builds before the frame-index calls)
            L.kcnn_corpus_new.restype = ctypes.c_void_p
            L.kcnn_corpus_new.argtypes = [ctypes.c_void_p, MatrixDim, ctypes.c_void_p,
                                          ctypes.c_int]
            L.kcnn_corpus_free.argtypes = [ctypes.c_void_p]
            L.kcnn_nnet_propagate_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_int]
            L.kcnn_nnet_compute_prob_frames.argtypes = [
                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        if hasattr(L, "kcnn_nnet_propagate_frames_shared"):  # (absent before time-shared training)
            L.kcnn_nnet_propagate_frames_shared.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                                            ctypes.c_void_p, ctypes.c_int]
            L.kcnn_nnet_time_train_prefix.argtypes = [ctypes.c_void_p]
        if hasattr(L, "kcnn_online_new"):  # (absent from builds before the streaming pass)
            L.kcnn_online_new.restype = ctypes.c_void_p
            L.kcnn_online_new.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                          ctypes.c_int]
            L.kcnn_online_free.argtypes = [ctypes.c_void_p]
        if hasattr(L, "kcnn_online_new_shared"):  # (absent from builds before share_time)
            L.kcnn_online_new_shared.restype = ctypes.c_void_p
            L.kcnn_online_new_shared.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                                 ctypes.c_int, ctypes.c_int]
            L.kcnn_online_shared_prefix.argtypes = [ctypes.c_void_p]
            L.kcnn_online_accept.argtypes = [
                ctypes.c_void_p, ctypes.c_void_p, MatrixDim, ctypes.c_void_p, ctypes.c_void_p,
                ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            L.kcnn_online_reset.argtypes = [ctypes.c_void_p, ctypes.c_int]
            L.kcnn_online_frames.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        if hasattr(L, "kcnn_nnet_xent_deriv"):  # (absent from builds before the DP xent step)
            L.kcnn_nnet_xent_deriv.argtypes = [
                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            L.kcnn_nnet_skip_dropout_call.argtypes = [ctypes.c_void_p]
            L.kcnn_nnet_set_row_offset.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
            L.kcnn_component_set_dropout_row_offset.argtypes = [ctypes.c_void_p,
                                                                ctypes.c_uint64]
        L.kcnn_nnet_free.argtypes = [ctypes.c_void_p]
        L.kcnn_nnet_component.restype = ctypes.c_void_p
        L.kcnn_nnet_component.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.kcnn_set_stream.argtypes = [ctypes.c_void_p]
        L.kcnn_set_randn_seed.argtypes = [ctypes.c_uint64]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise KcnnError(lib().kcnn_last_error().decode(errors="replace"))
    return rc


def declared_symbols():
    """Function names declared in include/*.h (the exported C-ABI)."""
    import re
    names = []
    for fn in sorted(os.listdir(INCLUDE_DIR)):
        if not fn.endswith(".h"):
            continue
        src = open(os.path.join(INCLUDE_DIR, fn)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names += re.findall(r"\b((?:hipF|kcnn)_[A-Za-z0-9_]+)\s*\(", src)
    return sorted(set(names))


# ---------------------------------------------------------------------------
# device / stream
_initialized_device = None


def init(device: int = 0):
    """CuDevice::SelectGpuId + bind the library to torch's current stream."""
    global _initialized_device
    import torch
    if not torch.cuda.is_available():
        raise KcnnError("no GPU: the kcnn product path has no CPU fallback")
    torch.cuda.set_device(device)
    check(lib().kcnn_init(device))
    sync_stream()
    _initialized_device = device


def sync_stream():
    """Launch subsequent kernels on torch's current stream."""
    import torch
    check(lib().kcnn_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _ensure_init():
    if _initialized_device is None:
        import torch
        init(torch.cuda.current_device() if torch.cuda.is_available() else 0)


def set_literal_path(on: bool):
    check(lib().kcnn_set_literal_path(int(bool(on))))


def set_profiling(on: bool):
    check(lib().kcnn_set_profiling(int(bool(on))))


def set_fusion(mode):
    """kcnn_nnet runtime: fuse Conv -> Maxpool (see kcnn.h).  0 / False: off;
    1 / True: on, the conv output not stored; 2: on, the conv output stored."""
    check(lib().kcnn_set_fusion(int(mode)))


def device_malloc_calls() -> int:
    """CuDevice::Malloc calls so far (kcnn_device_malloc_calls)."""
    return int(lib().kcnn_device_malloc_calls())


def conv_fix_counts(reset=False):
    """(f16x3 implicit-GEMM calls, tiles, elements recomputed by its fp32
    fix-ups) since the last reset (kcnn_conv_fix_counts)."""
    if not hasattr(lib(), "kcnn_conv_fix_counts"):  # (absent from pre-r06 builds)
        return None
    out = (ctypes.c_ulonglong * 3)()
    check(lib().kcnn_conv_fix_counts(out, int(bool(reset))))
    return tuple(int(v) for v in out)


def profile_string() -> str:
    buf = ctypes.create_string_buffer(1 << 16)
    check(lib().kcnn_profile_string(buf, len(buf)))
    return buf.value.decode()


def set_gemm_mode(mode: int):
    """AddMatMat's fp32 product: 0 = rocBLAS sgemm, 1 = bf16x6 split kernel,
    2 = f16x3 split kernel, tile by its cost model (default), 3 = f16x3 on the
    256 x 256 tile wherever a call can take it, 4 = f16x3 on the 256 x 128
    tile."""
    check(lib().kcnn_set_gemm_mode(int(mode)))


def gemm_tile_counts(reset=False):
    """(f16x3 GEMM launches on the 256 x 128 tile, on the 256 x 256 tile)
    since the last reset (kcnn_gemm_tile_counts)."""
    out = (ctypes.c_ulonglong * 2)()
    check(lib().kcnn_gemm_tile_counts(out, int(bool(reset))))
    return tuple(int(v) for v in out)


def gemm_plan(trans_a, trans_b, m, n, k, lda=None, ldb=None):
    """(tile columns, ksplit, nwhole) the f16x3 GEMM would give the call under
    the current "gemm" selector (kcnn_gemm_plan; no GPU needed).  lda / ldb
    default to the operands' dense pitches."""
    if lda is None:
        lda = m if trans_a else k
    if ldb is None:
        ldb = k if trans_b else n
    out = (ctypes.c_int * 3)()
    check(lib().kcnn_gemm_plan(int(bool(trans_a)), int(bool(trans_b)), int(m), int(n), int(k),
                               int(lda), int(ldb), out))
    return tuple(int(v) for v in out)


def gemm_fixup_counts(reset=False):
    """(split-K f16x3 GEMM calls that launched the fix-up kernel, calls that
    skipped it) since the last reset (kcnn_gemm_fixup_counts; no GPU needed)."""
    out = (ctypes.c_ulonglong * 2)()
    check(lib().kcnn_gemm_fixup_counts(out, int(bool(reset))))
    return tuple(int(v) for v in out)


def gemm_fixup_sites_reset():
    """Forget every fix-up call site: the next split-K call at any key launches
    the fix-up (kcnn_gemm_fixup_sites_reset; no GPU needed)."""
    check(lib().kcnn_gemm_fixup_sites_reset())


def set_kernel_family(name: str, value: int):
    """Kernel-family selector (kcnn.h): "fwd_x6" (2 f16x3 / 1 bf16x6 / 0),
    "bwd_x6", "igemm_x6", "wgrad_x6" (2 wide / 1 / 0) or "gemm" (2 f16x3 /
    3 f16x3 wide tile / 4 f16x3 narrow tile / 1 bf16x6 / 0 rocBLAS); 0 = the
    fp32-MFMA kernels."""
    check(lib().kcnn_set_kernel_family(name.encode(), int(value)))


def get_kernel_family(name: str) -> int:
    v = lib().kcnn_get_kernel_family(name.encode())
    if v < 0:
        raise KcnnError(f"unknown kernel family {name!r}")
    return v


def gemm(a, b, c, trans_a=False, trans_b=False, alpha=1.0, beta=0.0):
    """c = alpha * op(a) op(b) + beta * c (CuMatrixBase::AddMatMat) on torch
    fp32 device matrices with contiguous rows."""
    m, n = c.shape
    am, k = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    bk, bn = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if am != m or bk != k or bn != n:
        raise KcnnError(f"gemm: op(a) {am}x{k}, op(b) {bk}x{bn} do not make c {m}x{n}")
    for t in (a, b, c):
        dim(t)
    check(lib().kcnn_gemm(int(bool(trans_a)), int(bool(trans_b)), m, n, k,
                          ctypes.c_float(alpha), ctypes.c_void_p(a.data_ptr()), a.stride(0),
                          ctypes.c_void_p(b.data_ptr()), b.stride(0), ctypes.c_float(beta),
                          ctypes.c_void_p(c.data_ptr()), c.stride(0)))


def split_planes(x):
    """fp32 [rows x cols] device matrix -> int16 tensor [3, rows, cols'] of its
    bf16 planes h, m, l (x = h + m + l exactly); cols' = cols rounded up to 8."""
    import torch
    rows, cols = x.shape
    ldp = (cols + 7) // 8 * 8
    out = torch.zeros((3, rows, ldp), dtype=torch.int16, device=x.device)
    check(lib().kcnn_split_planes(ctypes.c_void_p(x.data_ptr()), rows, cols, x.stride(0),
                                  ctypes.c_void_p(out.data_ptr()), ldp,
                                  ctypes.c_int64(rows * ldp)))
    return out


def gemm_planes(ap, bp, c, k, trans_a=False, trans_b=False, alpha=1.0, beta=0.0):
    """kcnn_gemm from split_planes() operands; c fp32 [m x n]."""
    m, n = c.shape
    check(lib().kcnn_gemm_planes(int(bool(trans_a)), int(bool(trans_b)), m, n, k,
                                 ctypes.c_float(alpha), ctypes.c_void_p(ap.data_ptr()),
                                 ap.stride(1), ctypes.c_int64(ap.stride(0)),
                                 ctypes.c_void_p(bp.data_ptr()), bp.stride(1),
                                 ctypes.c_int64(bp.stride(0)), ctypes.c_float(beta),
                                 ctypes.c_void_p(c.data_ptr()), c.stride(0)))


def reset_profile():
    check(lib().kcnn_reset_profile())


def set_randn_seed(seed: int):
    lib().kcnn_set_randn_seed(ctypes.c_uint64(seed))


def synchronize():
    check(lib().kcnn_synchronize())


def dim(t) -> MatrixDim:
    assert t.dim() == 2, "matrices are 2-D"
    assert t.dtype.is_floating_point and t.element_size() == 4, t.dtype
    assert t.is_cuda, "device tensors only"
    assert t.shape[1] <= 1 or t.stride(1) == 1, "rows must be contiguous"
    stride = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    return MatrixDim(t.shape[0], t.shape[1], stride)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def empty(rows, cols, device=None):
    import torch
    return torch.empty((rows, cols), dtype=torch.float32,
                       device=device or "cuda")


def zeros(rows, cols, device=None):
    import torch
    return torch.zeros((rows, cols), dtype=torch.float32,
                       device=device or "cuda")


# ---------------------------------------------------------------------------
# CuMatrixBase extension methods (cu-matrix.h:451-480)

def Conv2D(this, kernel, in_height, in_width, in_channel, kernel_height,
           kernel_width, group, out=None, concat=True):
    _ensure_init()
    oh, ow = in_height - kernel_height + 1, in_width - kernel_width + 1
    if out is None:
        out = (empty(this.shape[0], oh * ow * group) if concat
               else empty(oh * ow * this.shape[0], group))
    check(lib().kcnn_mat_conv2d(ptr(this), dim(this), ptr(kernel), dim(kernel),
                                in_height, in_width, in_channel, kernel_height,
                                kernel_width, group, ptr(out), dim(out),
                                int(concat)))
    return out


def AddMatRepVec(this, vec, rep):
    _ensure_init()
    check(lib().kcnn_mat_add_mat_rep_vec(ptr(this), dim(this), ptr(vec),
                                         vec.numel(), rep))
    return this


def FlipMat(this, kernel_height, kernel_width, in_channel, group, flip=None):
    _ensure_init()
    if flip is None:
        flip = zeros(kernel_height * kernel_width * group, in_channel)
    check(lib().kcnn_mat_flip_mat(ptr(this), dim(this), kernel_height,
                                  kernel_width, in_channel, group, ptr(flip),
                                  dim(flip)))
    return flip


def PaddingZero(this, orig_height, orig_width, orig_channel, kernel_height,
                kernel_width, padmat=None):
    _ensure_init()
    ph, pw = orig_height + 2 * (kernel_height - 1), orig_width + 2 * (kernel_width - 1)
    if padmat is None:
        padmat = zeros(this.shape[0], ph * pw * orig_channel)
    check(lib().kcnn_mat_padding_zero(ptr(this), dim(this), orig_height,
                                      orig_width, orig_channel, kernel_height,
                                      kernel_width, ptr(padmat), dim(padmat)))
    return padmat


def TpBlock(this, in_channel, block_size, out=None):
    _ensure_init()
    if out is None:
        out = zeros(in_channel, this.shape[0] * block_size)
    check(lib().kcnn_mat_tp_block(ptr(this), dim(this), in_channel, block_size,
                                  ptr(out), dim(out)))
    return out


def TpInsideBlock(this, group, block_size, out=None):
    _ensure_init()
    if out is None:
        out = zeros(block_size * this.shape[0], group)
    check(lib().kcnn_mat_tp_inside_block(ptr(this), dim(this), group,
                                         block_size, ptr(out), dim(out)))
    return out


def ModPermuteRow(this, in_channel, block_size, out=None):
    _ensure_init()
    if out is None:
        out = zeros(this.shape[0], this.shape[1])
    check(lib().kcnn_mat_mod_permute_row(ptr(this), dim(this), in_channel,
                                         block_size, ptr(out), dim(out)))
    return out


def ModPermuteChannel(this, comp_idx, num_component, in_height, in_width,
                      container, from_comp_to_container):
    """conv2D.cc:685-727; writes `container` (or `this` when
    from_comp_to_container is False)."""
    _ensure_init()
    check(lib().kcnn_mat_mod_permute_channel(
        ptr(this), dim(this), comp_idx, num_component, in_height, in_width,
        ptr(container), dim(container), int(bool(from_comp_to_container))))
    return container if from_comp_to_container else this


def Maxpool_prop(this, in_height, in_width, pool_height_dim, pool_width_dim,
                 pool_channel_dim, overlap, overlap2D, out):
    _ensure_init()
    check(lib().kcnn_mat_maxpool_prop(ptr(this), dim(this), in_height, in_width,
                                      pool_height_dim, pool_width_dim,
                                      pool_channel_dim, int(overlap),
                                      int(overlap2D), ptr(out), dim(out)))
    return out


def Maxpool_backprop(this, out_value, out_deriv, in_deriv, in_height, in_width,
                     pool_height_dim, pool_width_dim, pool_channel_dim,
                     overlap=False, overlap2D=False):
    _ensure_init()
    check(lib().kcnn_mat_maxpool_backprop(
        ptr(this), dim(this), ptr(out_value), dim(out_value), ptr(out_deriv),
        dim(out_deriv), ptr(in_deriv), dim(in_deriv), in_height, in_width,
        pool_height_dim, pool_width_dim, pool_channel_dim, int(overlap),
        int(overlap2D)))
    return in_deriv


# ---------------------------------------------------------------------------
# Components

PARAM_LINEAR, PARAM_BIAS, PARAM_PREV_GRAD = 0, 1, 2


class Component:
    """Handle on an nnet2 component living in libkcnn.so."""

    def __init__(self, handle, owned=True, keep=None):
        if not handle:
            raise KcnnError(lib().kcnn_last_error().decode(errors="replace"))
        self._h = ctypes.c_void_p(handle)
        self._owned = owned
        self._keep = keep  # keeps an owning Nnet alive for borrowed handles

    @classmethod
    def NewFromString(cls, initializer_line: str) -> "Component":
        _ensure_init()
        return cls(lib().kcnn_component_new_from_string(initializer_line.encode()))

    @classmethod
    def ReadNew(cls, path: str) -> "Component":
        _ensure_init()
        return cls(lib().kcnn_component_read(str(path).encode()))

    def Write(self, path: str, binary: bool = True):
        check(lib().kcnn_component_write(self._h, str(path).encode(), int(binary)))

    def Copy(self) -> "Component":
        return Component(lib().kcnn_component_copy(self._h))

    def __del__(self):
        try:
            if getattr(self, "_owned", False) and self._h:
                lib().kcnn_component_free(self._h)
                self._h = None
        except Exception:
            pass

    def _str(self, fn) -> str:
        buf = ctypes.create_string_buffer(4096)
        check(fn(self._h, buf, len(buf)))
        return buf.value.decode()

    def SplitGradient(self) -> bool:
        """Whether kcnn_dp may compute this layer's gradient apart from its
        data gradient (mode 3 then mode 2): not for a convolution, whose
        fused backward makes both from one pass over its output derivative."""
        return self.Type() != "ConvolutionComponent"

    def Type(self) -> str:
        return self._str(lib().kcnn_component_type)

    def Info(self) -> str:
        return self._str(lib().kcnn_component_info)

    def InputDim(self) -> int:
        return lib().kcnn_component_input_dim(self._h)

    def OutputDim(self) -> int:
        return lib().kcnn_component_output_dim(self._h)

    def BackpropNeedsInput(self) -> bool:
        return bool(lib().kcnn_component_backprop_needs_input(self._h))

    def BackpropNeedsOutput(self) -> bool:
        return bool(lib().kcnn_component_backprop_needs_output(self._h))

    def Context(self):
        """Component::Context(): frame offsets read per output frame."""
        buf = (ctypes.c_int * 256)()
        n = lib().kcnn_component_context(self._h, buf, 256)
        if n < 0:
            check(1)
        return list(buf[:n])

    def _span(self):
        ctx = self.Context()
        return ctx[-1] - ctx[0]

    def Propagate(self, inp, out=None, num_chunks=None):
        """num_chunks defaults to one output frame per chunk (the input chunk
        is that frame widened by Context(): SpliceComponent)."""
        span = self._span()
        if num_chunks is None:
            num_chunks = inp.shape[0] // (span + 1)
        if out is None:
            out = empty(inp.shape[0] - num_chunks * span, self.OutputDim())
        check(lib().kcnn_component_propagate(self._h, ptr(inp), dim(inp),
                                             ptr(out), dim(out), num_chunks))
        return out

    def NonlinearStats(self):
        """(value_sum, deriv_sum, count) of a NonlinearComponent (fp64)."""
        import numpy as np
        n = self.InputDim()
        vs, ds = np.zeros(n, np.float64), np.zeros(n, np.float64)
        cnt = ctypes.c_double()
        k = ctypes.c_int()
        check(lib().kcnn_component_nonlinear_stats(
            self._h, vs.ctypes.data_as(ctypes.c_void_p), ds.ctypes.data_as(ctypes.c_void_p),
            n, ctypes.byref(k), ctypes.byref(cnt)))
        return vs[:k.value], ds[:k.value], cnt.value

    def Backprop(self, in_value, out_value, out_deriv, in_deriv=None,
                 update=True, num_chunks=None, need_in_deriv=True):
        span = self._span()
        if num_chunks is None:
            num_chunks = out_deriv.shape[0]
        if in_deriv is None and need_in_deriv:
            in_deriv = empty(out_deriv.shape[0] + num_chunks * span, self.InputDim())
        if out_value is None:
            out_value = out_deriv  # dummy when BackpropNeedsOutput() is false
        if in_value is None:
            in_value = in_deriv if in_deriv is not None else out_deriv
        idim = dim(in_deriv) if in_deriv is not None else MatrixDim(0, 0, 0)
        check(lib().kcnn_component_backprop(
            self._h, ptr(in_value), dim(in_value), ptr(out_value),
            dim(out_value), ptr(out_deriv), dim(out_deriv), ptr(in_deriv), idim,
            num_chunks, int(update)))
        return in_deriv

    # parameters
    def ParamDim(self, which):
        r, c = ctypes.c_int(), ctypes.c_int()
        check(lib().kcnn_component_param_dim(self._h, which, ctypes.byref(r),
                                             ctypes.byref(c)))
        return r.value, c.value

    def GetParam(self, which):
        r, c = self.ParamDim(which)
        t = empty(r, c)
        check(lib().kcnn_component_get_param(self._h, which, ptr(t), dim(t)))
        return t if which != PARAM_BIAS else t.view(-1)

    def SetParam(self, which, value):
        r, c = self.ParamDim(which)
        v = value.reshape(r, c).contiguous().float()
        check(lib().kcnn_component_set_param(self._h, which, ptr(v), dim(v)))

    def LinearParams(self):
        return self.GetParam(PARAM_LINEAR)

    def BiasParams(self):
        return self.GetParam(PARAM_BIAS)

    def PrevGrad(self):
        return self.GetParam(PARAM_PREV_GRAD)

    def LearningRate(self) -> float:
        return lib().kcnn_component_learning_rate(self._h)

    def SetLearningRate(self, lr: float):
        check(lib().kcnn_component_set_learning_rate(self._h, ctypes.c_float(lr)))

    def DotProduct(self, other) -> float:
        out = ctypes.c_float()
        check(lib().kcnn_component_dot_product(self._h, other._h, ctypes.byref(out)))
        return out.value

    def SetZero(self, treat_as_gradient: bool):
        check(lib().kcnn_component_set_zero(self._h, int(treat_as_gradient)))

    def Scale(self, s: float):
        check(lib().kcnn_component_scale(self._h, ctypes.c_float(s)))

    def Add(self, alpha: float, other):
        check(lib().kcnn_component_add(self._h, ctypes.c_float(alpha), other._h))

    def PerturbParams(self, stddev: float):
        check(lib().kcnn_component_perturb_params(self._h, ctypes.c_float(stddev)))

    def NumGradientParams(self) -> int:
        return lib().kcnn_component_num_gradient_params(self._h)

    def ComputeGradient(self, in_value, out_deriv, grad=None):
        import torch
        if grad is None:
            grad = torch.empty(self.NumGradientParams(), dtype=torch.float32,
                               device="cuda")
        check(lib().kcnn_component_compute_gradient(
            self._h, ptr(in_value), dim(in_value), ptr(out_deriv),
            dim(out_deriv), ptr(grad)))
        return grad

    def BackpropGradient(self, in_value, out_deriv, in_deriv=None, grad=None,
                         want_in_deriv=True):
        """Backprop (no update) + ComputeGradient in one call; returns
        (in_deriv or None, grad)."""
        import torch
        if grad is None:
            grad = torch.empty(self.NumGradientParams(), dtype=torch.float32,
                               device="cuda")
        if in_deriv is None and want_in_deriv:
            in_deriv = empty(in_value.shape[0], self.InputDim())
        check(lib().kcnn_component_backprop_gradient(
            self._h, ptr(in_value), dim(in_value), ptr(out_deriv),
            dim(out_deriv), ptr(in_deriv) if in_deriv is not None else None,
            dim(in_deriv) if in_deriv is not None else MatrixDim(0, 0, 0),
            ptr(grad)))
        return in_deriv, grad

    def ApplyGradient(self, grad, num_sample: int):
        check(lib().kcnn_component_apply_gradient(self._h, ptr(grad), int(num_sample)))

    def FlipKernelBranch(self) -> bool:
        rc = lib().kcnn_component_conv_flip_branch(self._h)
        if rc < 0:
            check(rc)
        return bool(rc)

    # DropoutComponent
    def SetDropoutScale(self, scale: float):
        """DropoutComponent::SetDropoutScale; 1.0 is inference (identity)."""
        check(lib().kcnn_component_set_dropout_scale(self._h, ctypes.c_float(scale)))

    def DropoutSeed(self) -> int:
        seed = ctypes.c_uint64()
        check(lib().kcnn_component_dropout_seed(self._h, ctypes.byref(seed)))
        return seed.value

    def SetDropoutSeed(self, seed: int):
        """Sets the mask generator's seed and restarts its call count: the
        mask of Propagate call k is a function of (seed, k, row, column)."""
        check(lib().kcnn_component_set_dropout_seed(self._h, ctypes.c_uint64(seed)))

    def SetDropoutRowOffset(self, offset: int):
        """The row of the minibatch that row 0 of Propagate's input is
        (kcnn_component_set_dropout_row_offset): the mask of row r is drawn
        for row offset + r.  Not written to files; a Copy() starts at 0."""
        if not 0 <= int(offset) < 1 << 64:
            raise KcnnError(f"SetDropoutRowOffset: offset {offset}")
        check(lib().kcnn_component_set_dropout_row_offset(self._h, ctypes.c_uint64(int(offset))))


def _label_arrays(labels):
    """labels: a sequence of (row, col, weight) triples (the reference's
    std::vector<MatrixElement>), or a tuple of three arrays (rows, cols,
    weights) -> contiguous int32, int32, float32 host arrays."""
    import numpy as np
    if isinstance(labels, tuple) and len(labels) == 3 and np.ndim(labels[0]) == 1:
        rows, cols, weights = labels
    else:
        a = np.asarray(labels, np.float64).reshape(-1, 3)
        rows, cols, weights = a[:, 0], a[:, 1], a[:, 2]
    rows = np.ascontiguousarray(rows, np.int32)
    cols = np.ascontiguousarray(cols, np.int32)
    weights = np.ascontiguousarray(weights, np.float32)
    if not (rows.shape == cols.shape == weights.shape):
        raise KcnnError("labels: rows, cols and weights differ in length")
    return rows, cols, weights


def comp_objf_and_deriv(probs, labels, deriv):
    """CuMatrix::CompObjfAndDeriv: deriv(row, col) += weight / probs(row, col)
    for the (row, col, weight) elements of `labels` (host; see
    Nnet.BackpropXent); returns (tot_objf, tot_weight)."""
    _ensure_init()
    rows, cols, weights = _label_arrays(labels)
    objf, weight = ctypes.c_double(), ctypes.c_double()
    check(lib().kcnn_comp_objf_and_deriv(
        rows.ctypes.data_as(ctypes.c_void_p), cols.ctypes.data_as(ctypes.c_void_p),
        weights.ctypes.data_as(ctypes.c_void_p), len(rows), ptr(probs), dim(probs),
        ptr(deriv), dim(deriv), ctypes.byref(objf), ctypes.byref(weight)))
    return objf.value, weight.value


def comp_objf_accuracy(probs, labels):
    """The objective and frame accuracy of nnet-compute-prob on a device
    matrix (kcnn_comp_objf_accuracy): for the (row, col, weight) elements of
    `labels` (host) returns (sum of weight * log probs(row, col), sum of
    weight, sum of the weights of the elements whose column is their row's
    best column)."""
    _ensure_init()
    rows, cols, weights = _label_arrays(labels)
    out = (ctypes.c_double * 3)()
    check(lib().kcnn_comp_objf_accuracy(
        rows.ctypes.data_as(ctypes.c_void_p), cols.ctypes.data_as(ctypes.c_void_p),
        weights.ctypes.data_as(ctypes.c_void_p), len(rows), ptr(probs), dim(probs), out))
    return out[0], out[1], out[2]


class Nnet:
    """A stack of components run like upstream nnet2's NnetUpdater."""

    def __init__(self, config: str):
        _ensure_init()
        self._adopt(lib().kcnn_nnet_new(config.encode()))

    def _adopt(self, h):
        self._h = None
        if not h:
            raise KcnnError(lib().kcnn_last_error().decode(errors="replace"))
        self._h = ctypes.c_void_p(h)
        n = lib().kcnn_nnet_num_components(self._h)
        self.components = [Component(lib().kcnn_nnet_component(self._h, i),
                                     owned=False, keep=self) for i in range(n)]

    @classmethod
    def _from_handle(cls, h) -> "Nnet":
        net = cls.__new__(cls)
        net._adopt(h)
        return net

    @classmethod
    def Read(cls, path: str) -> "Nnet":
        """A whole network from a Kaldi <Nnet> stream file, binary or text
        (kcnn_nnet_read; upstream Nnet::Read)."""
        _ensure_init()
        return cls._from_handle(lib().kcnn_nnet_read(str(path).encode()))

    def Write(self, path: str, binary: bool = True):
        """The network as a Kaldi <Nnet> stream file (upstream Nnet::Write)."""
        check(lib().kcnn_nnet_write(self._h, str(path).encode(), int(bool(binary))))

    def Copy(self, scales=None, remove_dropout=False) -> "Nnet":
        """nnet-am-copy: a new network of copies of the components.  scales:
        one factor per updatable component (--scales); remove_dropout: leave
        the DropoutComponents out (--remove-dropout).  Both together give the
        test model of the dropout recipes."""
        import numpy as np
        p, n = None, 0
        if scales is not None:
            s = np.ascontiguousarray(scales, np.float32).ravel()
            p, n = s.ctypes.data_as(ctypes.c_void_p), len(s)
        return Nnet._from_handle(lib().kcnn_nnet_copy(self._h, p, n, int(bool(remove_dropout))))

    def __del__(self):
        try:
            if self._h:
                lib().kcnn_nnet_free(self._h)
                self._h = None
        except Exception:
            pass

    def NumComponents(self):
        return len(self.components)

    def Propagate(self, inp):
        self._input = inp  # the library borrows it until Backprop
        check(lib().kcnn_nnet_propagate(self._h, ptr(inp), dim(inp)))

    def Output(self, i=-2):
        """Layer i's output as a torch view (i = -2: the last layer)."""
        import torch
        if i == -2:
            i = self.NumComponents() - 1
        p = ctypes.c_void_p()
        d = MatrixDim()
        check(lib().kcnn_nnet_output(self._h, i, ctypes.byref(p), ctypes.byref(d)))
        return _device_view(p.value, d)

    def InputDeriv(self, i):
        """d(input of component i) from the last backprop, as a torch view."""
        p = ctypes.c_void_p()
        d = MatrixDim()
        check(lib().kcnn_nnet_input_deriv(self._h, i, ctypes.byref(p), ctypes.byref(d)))
        return _device_view(p.value, d)

    def BackpropComponent(self, i, out_deriv=None, mode=0, grad=None,
                          skip_first_dx=True):
        od = out_deriv
        odim = dim(od) if od is not None else MatrixDim(0, 0, 0)
        check(lib().kcnn_nnet_backprop_component(self._h, i, ptr(od), odim, mode,
                                                 ptr(grad), int(skip_first_dx)))

    def BackpropSplit(self, i, out_deriv, grad, skip_first_dx, between):
        """kcnn_nnet_backprop_split: affine layer i's gradient into grad,
        then between() (e.g. the gradient's all-reduce is started there),
        then its input derivative; one statistics pass for both GEMMs."""
        err = []

        def cb(_ctx):
            try:
                between()
            except BaseException as e:  # noqa: BLE001 -- re-raised below
                err.append(e)
        fn = ctypes.CFUNCTYPE(None, ctypes.c_void_p)(cb)
        od = out_deriv
        odim = dim(od) if od is not None else MatrixDim(0, 0, 0)
        rc = lib().kcnn_nnet_backprop_split(self._h, i, ptr(od), odim, ptr(grad),
                                            int(skip_first_dx), fn, None)
        if err:
            raise err[0]
        check(rc)

    def Backprop(self, out_deriv, skip_first_dx=False):
        """The whole backward in one kcnn_nnet_backprop call; with
        skip_first_dx, one kcnn_nnet_backprop_component call per layer."""
        if not skip_first_dx:
            check(lib().kcnn_nnet_backprop(self._h, ptr(out_deriv), dim(out_deriv)))
            return
        for i in reversed(range(self.NumComponents())):
            self.BackpropComponent(i, out_deriv, 0, None, skip_first_dx)

    def BackpropXent(self, labels, skip_first_dx=False):
        """The backward of a training step from labels (kcnn_nnet_backprop_xent):
        `labels` are (row, col, weight) elements of the last Propagate's
        output, sorted by row, as a sequence of triples or a tuple of three
        arrays.  Adds to the totals ObjfTotal returns; does not synchronise."""
        rows, cols, weights = _label_arrays(labels)
        check(lib().kcnn_nnet_backprop_xent(
            self._h, rows.ctypes.data_as(ctypes.c_void_p),
            cols.ctypes.data_as(ctypes.c_void_p), weights.ctypes.data_as(ctypes.c_void_p),
            len(rows), int(skip_first_dx)))

    def XentDeriv(self, labels):
        """The first half of BackpropXent (kcnn_nnet_xent_deriv), for a caller
        that runs the backward itself: checks and stages `labels`, adds to the
        totals ObjfTotal returns, and leaves the output derivative in the
        library.  Returns (first, out_deriv): the component the backward
        starts at, and what to pass to BackpropComponent / BackpropSplit as
        out_deriv -- a torch view, or None when a last Softmax took the fused
        kernel (first is then NumComponents() - 2, and a backprop call of the
        last component raises).  Does not synchronise."""
        rows, cols, weights = _label_arrays(labels)
        first = ctypes.c_int()
        p = ctypes.c_void_p()
        d = MatrixDim()
        check(lib().kcnn_nnet_xent_deriv(
            self._h, rows.ctypes.data_as(ctypes.c_void_p),
            cols.ctypes.data_as(ctypes.c_void_p), weights.ctypes.data_as(ctypes.c_void_p),
            len(rows), ctypes.byref(first), ctypes.byref(p), ctypes.byref(d)))
        return first.value, (_device_view(p.value, d) if p.value else None)

    def SetRowOffset(self, offset: int):
        """Component.SetDropoutRowOffset on every DropoutComponent of the
        stack (kcnn_nnet_set_row_offset); holds until set again."""
        if not 0 <= int(offset) < 1 << 64:
            raise KcnnError(f"SetRowOffset: offset {offset}")
        check(lib().kcnn_nnet_set_row_offset(self._h, ctypes.c_uint64(int(offset))))

    def SkipDropoutCall(self):
        """Every DropoutComponent counts a Propagate call that did not run
        here (kcnn_nnet_skip_dropout_call): a data-parallel rank with an empty
        shard keeps the call number, and so the masks, of the others."""
        check(lib().kcnn_nnet_skip_dropout_call(self._h))

    def ObjfTotal(self, reset=False):
        """(sum of weight * log-probability, sum of weight) over the
        BackpropXent / XentDeriv calls since the last reset; synchronises."""
        out = (ctypes.c_double * 2)()
        check(lib().kcnn_nnet_objf_total(self._h, out, int(bool(reset))))
        return out[0], out[1]

    def ComputeProb(self, inp, labels):
        """nnet-compute-prob on one minibatch (kcnn_nnet_compute_prob): the
        forward pass over `inp`, then the objective, weight and accuracy
        weight of `labels` (as for BackpropXent) added to the totals ProbTotal
        returns.  Changes nothing in the network and does not synchronise;
        Backprop* raise until the next Propagate."""
        rows, cols, weights = _label_arrays(labels)
        self._input = inp
        check(lib().kcnn_nnet_compute_prob(
            self._h, ptr(inp), dim(inp), rows.ctypes.data_as(ctypes.c_void_p),
            cols.ctypes.data_as(ctypes.c_void_p), weights.ctypes.data_as(ctypes.c_void_p),
            len(rows)))

    def ProbTotal(self, reset=False):
        """(sum of weight * log-probability, sum of weight, accuracy weight)
        over the ComputeProb calls since the last reset; synchronises."""
        out = (ctypes.c_double * 3)()
        check(lib().kcnn_nnet_prob_total(self._h, out, int(bool(reset))))
        return out[0], out[1], out[2]

    def LeftContext(self):
        """The frames the network reads before the frame it computes
        (upstream Nnet::LeftContext)."""
        return lib().kcnn_nnet_left_context(self._h)

    def RightContext(self):
        """The frames it reads after that frame (Nnet::RightContext)."""
        return lib().kcnn_nnet_right_context(self._h)

    def TimeSharedPrefix(self):
        """The number of leading components Compute(share_time=True) runs once
        per time step (kcnn_nnet_time_shared_prefix); 0: it runs Compute's own
        pass."""
        return lib().kcnn_nnet_time_shared_prefix(self._h)

    def TimeMap(self, level):
        """Level `level` of the last Compute(share_time=True)
        (kcnn_nnet_time_map): (torch view of its computed rows, one per input
        row, by height * channels (TimeMapHeight); channels; positions;
        dilation).  Valid until the
        next forward call; for tests and debugging."""
        p = ctypes.c_void_p()
        d = MatrixDim()
        c, n, dil = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().kcnn_nnet_time_map(self._h, int(level), ctypes.byref(p), ctypes.byref(d),
                                       ctypes.byref(c), ctypes.byref(n), ctypes.byref(dil)))
        return _device_view(p.value, d), c.value, n.value, dil.value

    def TimeMapHeight(self, level):
        """The height H of that level (kcnn_nnet_time_map_height): a row of
        TimeMap(level)'s view holds H * channels floats, element (h, c) at
        column h + c * H; 1 for a level without a frequency axis."""
        h = ctypes.c_int()
        check(lib().kcnn_nnet_time_map_height(self._h, int(level), ctypes.byref(h)))
        return h.value

    def Compute(self, feats, lengths=None, pad_input=True, priors=None, prior_scale=1.0,
                apply_log=False, share_time=False):
        """The forward pass of upstream NnetComputer (nnet-am-compute, the
        decodable) on whole utterances (kcnn_nnet_compute).  `feats`: the
        utterances' frames stacked row-wise in one device matrix; `lengths`:
        their frame counts (host; None: one utterance).  With pad_input each
        utterance is padded with copies of its first and last frame by
        LeftContext() / RightContext() and gives one row per frame; without,
        it gives LeftContext() + RightContext() fewer rows.  apply_log: the
        log of the output, minus prior_scale * log(priors) when `priors` (one
        per output, host) are given.  Returns a torch view of the result,
        valid until the next forward call; changes nothing in the network and
        does not synchronise; Backprop* raise until the next Propagate.
        share_time (kcnn_nnet_compute_shared): the leading Splice ->
        {Convolution | Maxpool | ReLU}... components (convolutions along time,
        along frequency or both; stride 1, no padding) run once per time step
        instead of once per window -- the same values to the error bar of the
        GEMMs, not the same bits; Output(i) of those components but the last
        then raises, TimeMap gives their maps.  A network this does not cover
        (TimeSharedPrefix() == 0) runs as without it."""
        import numpy as np
        if lengths is None:
            lengths = [feats.shape[0]]
        try:
            lens = np.ascontiguousarray(lengths, np.int32).ravel()
        except (OverflowError, ValueError) as e:
            raise KcnnError(f"Compute: bad lengths: {e}") from None
        pp, np_ = None, 0
        if priors is not None:
            pr = np.ascontiguousarray(priors, np.float32).ravel()
            pp, np_ = pr.ctypes.data_as(ctypes.c_void_p), len(pr)
        self._input = feats  # the library borrows it as Propagate does
        p = ctypes.c_void_p()
        d = MatrixDim()
        fn = lib().kcnn_nnet_compute_shared if share_time else lib().kcnn_nnet_compute
        check(fn(
            self._h, ptr(feats), dim(feats), lens.ctypes.data_as(ctypes.c_void_p), len(lens),
            int(bool(pad_input)), pp, np_, ctypes.c_float(prior_scale), int(bool(apply_log)),
            ctypes.byref(p), ctypes.byref(d)))
        return _device_view(p.value, d)

    def PropagateFrames(self, corpus: "Corpus", frames, share_time=False):
        """Propagate on a minibatch given as rows of a device-resident corpus
        (kcnn_nnet_propagate_frames).  `frames`: host int32 indices of corpus
        rows, any order, repeats allowed; example n is frames[n], and its
        context window (clamped at its utterance's ends) is gathered on the
        device.  Output row n, and the labels' rows of a following
        BackpropXent, are example n.  Does not synchronise.
        share_time (kcnn_nnet_propagate_frames_shared): the leading
        TimeSharedTrainPrefix() components run once per time step of each run
        of consecutive rows in the list (time maps) instead of once per
        example's window, and Backprop / BackpropXent run their backward once
        over the maps -- the same step to the error bar of the GEMMs, not the
        same bits.  Output(i) of those components but the last then raises, as
        do BackpropComponent and InputDeriv of them; their ReLUs accumulate no
        statistics in such a step.  TimeMap, TimeMapDeriv and TimeGradient show
        the maps, their derivatives and the gradients applied.  Any list is
        legal; the saving grows with the length of its runs.  A network this
        does not cover (TimeSharedTrainPrefix() == 0) runs as without it."""
        fr = _frame_array(frames)
        self._input = corpus  # the library borrows its matrix until Backprop
        fn = (lib().kcnn_nnet_propagate_frames_shared if share_time
              else lib().kcnn_nnet_propagate_frames)
        check(fn(self._h, corpus._h, fr.ctypes.data_as(ctypes.c_void_p), len(fr)))

    def TimeSharedTrainPrefix(self):
        """The number of leading components PropagateFrames(share_time=True)
        runs as time maps (kcnn_nnet_time_train_prefix): TimeSharedPrefix(), or
        0 when one of them keeps a frequency axis."""
        return lib().kcnn_nnet_time_train_prefix(self._h)

    def TimeMapDeriv(self, level):
        """The derivative map of `level` after PropagateFrames(share_time=True)
        and a backward pass (kcnn_nnet_time_map_deriv), as TimeMap gives the
        map: (torch view, channels, positions, dilation).  Level 0 and a
        Maxpool's own level under a ReLU have none and raise.  Valid until the
        next forward call; for tests and debugging."""
        p = ctypes.c_void_p()
        d = MatrixDim()
        c, n, dil = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().kcnn_nnet_time_map_deriv(self._h, int(level), ctypes.byref(p),
                                             ctypes.byref(d), ctypes.byref(c), ctypes.byref(n),
                                             ctypes.byref(dil)))
        return _device_view(p.value, d), c.value, n.value, dil.value

    def TimeGradient(self, i):
        """The flat gradient that backward applied to Convolution i of the
        prefix (kcnn_nnet_time_gradient): a torch view of KernelDim * Group
        weight entries, row-major, then Group biases, ComputeGradient's
        layout."""
        p = ctypes.c_void_p()
        n = ctypes.c_int()
        check(lib().kcnn_nnet_time_gradient(self._h, int(i), ctypes.byref(p), ctypes.byref(n)))
        return _device_view(p.value, MatrixDim(1, n.value, n.value))[0]

    def ComputeProbFrames(self, corpus: "Corpus", frames, labels):
        """ComputeProb on such a minibatch (kcnn_nnet_compute_prob_frames);
        the labels' rows are 0 .. len(frames) - 1."""
        fr = _frame_array(frames)
        rows, cols, weights = _label_arrays(labels)
        self._input = corpus
        check(lib().kcnn_nnet_compute_prob_frames(
            self._h, corpus._h, fr.ctypes.data_as(ctypes.c_void_p), len(fr),
            rows.ctypes.data_as(ctypes.c_void_p), cols.ctypes.data_as(ctypes.c_void_p),
            weights.ctypes.data_as(ctypes.c_void_p), len(rows)))


def _frame_array(frames):
    import numpy as np
    try:
        return np.ascontiguousarray(frames, np.int32).ravel()
    except (OverflowError, ValueError) as e:
        raise KcnnError(f"bad frame indices: {e}") from None


class Corpus:
    """A training corpus that stays on the device (kcnn_corpus): `feats`, the
    [sum(lengths) x InputDim] device matrix of whole utterances stacked
    row-wise (borrowed by the library, kept alive here), and `lengths`, their
    frame counts (host ints).  Nnet.PropagateFrames / ComputeProbFrames take
    minibatches of its rows."""

    def __init__(self, feats, lengths):
        import numpy as np
        _ensure_init()
        self._h = None
        try:
            lens = np.ascontiguousarray(lengths, np.int32).ravel()
        except (OverflowError, ValueError) as e:
            raise KcnnError(f"Corpus: bad lengths: {e}") from None
        self.feats = feats
        self.lengths = lens
        h = lib().kcnn_corpus_new(ptr(feats), dim(feats),
                                  lens.ctypes.data_as(ctypes.c_void_p), len(lens))
        if not h:
            raise KcnnError(lib().kcnn_last_error().decode(errors="replace"))
        self._h = ctypes.c_void_p(h)

    def NumRows(self) -> int:
        return int(self.feats.shape[0])

    def __del__(self):
        try:
            if self._h:
                lib().kcnn_corpus_free(self._h)
                self._h = None
        except Exception:
            pass


class OnlineComputer:
    """The streaming forward pass over `num_streams` concurrent utterances
    (kcnn_online_*; upstream NnetOnlineComputer with pad_input): each Accept
    gives some slots their next frames, at most `max_chunk` each, and returns
    the rows that became computable.  `priors`, `prior_scale` and `apply_log`
    are Compute's.  `net` (the test model) is borrowed and kept alive here; the
    streams' history lives in device buffers of the computer's own, allocated
    by the first accepted step, so other forward calls of `net` between steps
    disturb nothing.  With `share_time` (kcnn_online_new_shared) a step runs
    the leading Splice -> Convolution / Maxpool / ReLU components once per time
    step of the frames its slots hold instead of once per emitted frame's
    window, where the network allows it (TimeSharedPrefix() > 0): the same
    rows to the error bar of the products, not the bits."""

    def __init__(self, net: Nnet, num_streams: int, max_chunk: int, priors=None,
                 prior_scale=1.0, apply_log=False, share_time=False):
        import numpy as np
        self._h = None
        self.net = net
        pp, np_ = None, 0
        if priors is not None:
            pr = np.ascontiguousarray(priors, np.float32).ravel()
            pp, np_ = pr.ctypes.data_as(ctypes.c_void_p), len(pr)
        if share_time:
            h = lib().kcnn_online_new_shared(net._h, int(num_streams), int(max_chunk), pp, np_,
                                             ctypes.c_float(prior_scale), int(bool(apply_log)),
                                             1)
        else:
            h = lib().kcnn_online_new(net._h, int(num_streams), int(max_chunk), pp, np_,
                                      ctypes.c_float(prior_scale), int(bool(apply_log)))
        if not h:
            raise KcnnError(lib().kcnn_last_error().decode(errors="replace"))
        self._h = ctypes.c_void_p(h)

    def __del__(self):
        try:
            if self._h:
                lib().kcnn_online_free(self._h)
                self._h = None
        except Exception:
            pass

    def Accept(self, chunk, streams, num_new, final):
        """One step (kcnn_online_accept).  `chunk`: the [sum(num_new) x
        InputDim] device matrix of the named slots' new frames, in the order
        of `streams` (None for a step of pure flushes); `streams`, `num_new`,
        `final`: host sequences, one entry per named slot, each slot at most
        once; num_new 0 only with final, which ends the utterance and frees
        the slot.  Returns (out, counts): `out` the rows that became
        computable -- a torch view valid until the next forward call of the
        net -- slots in the step's order, frames ascending, and `counts` the
        rows of each slot, so torch.split(out, counts) gives them per slot.
        Does not synchronise."""
        import numpy as np
        try:
            st = np.ascontiguousarray(streams, np.int32).ravel()
            nn = np.ascontiguousarray(num_new, np.int32).ravel()
            fi = np.ascontiguousarray([bool(f) for f in final], np.int32).ravel()
        except (OverflowError, ValueError, TypeError) as e:
            raise KcnnError(f"Accept: bad stream arrays: {e}") from None
        if not len(st) == len(nn) == len(fi):
            raise KcnnError(f"Accept: {len(st)} streams, {len(nn)} num_new, {len(fi)} final")
        counts = np.zeros(len(st), np.int32)
        self._chunk = chunk  # read by the step's kernel on the stream
        d = dim(chunk) if chunk is not None else MatrixDim(0, 0, 0)
        p = ctypes.c_void_p()
        od = MatrixDim()
        check(lib().kcnn_online_accept(
            self._h, ptr(chunk), d, st.ctypes.data_as(ctypes.c_void_p),
            nn.ctypes.data_as(ctypes.c_void_p), fi.ctypes.data_as(ctypes.c_void_p), len(st),
            counts.ctypes.data_as(ctypes.c_void_p), ctypes.byref(p), ctypes.byref(od)))
        return _device_view(p.value, od), [int(c) for c in counts]

    def TimeSharedPrefix(self):
        """The number of leading components the next step would run as time
        maps (kcnn_online_shared_prefix): 0 without share_time, or when the
        network's plan declines as the literal path now stands."""
        if not hasattr(lib(), "kcnn_online_shared_prefix"):
            return 0
        n = lib().kcnn_online_shared_prefix(self._h)
        if n < 0:
            raise KcnnError(lib().kcnn_last_error().decode(errors="replace"))
        return int(n)

    def Reset(self, stream: int):
        """Abandons the slot's utterance (kcnn_online_reset)."""
        check(lib().kcnn_online_reset(self._h, int(stream)))

    def Frames(self, stream: int):
        """(frames seen, rows emitted) of the slot's utterance."""
        out = (ctypes.c_int64 * 2)()
        check(lib().kcnn_online_frames(self._h, int(stream), out))
        return int(out[0]), int(out[1])


def chunk_runs(lengths, chunk):
    """The runs train_epoch(chunk=k) cuts a corpus into: every utterance in
    order as (first corpus row, rows) stretches of `chunk` consecutive rows,
    its last one possibly shorter."""
    runs, start = [], 0
    for t in lengths:
        t = int(t)
        runs += [(start + at, min(chunk, t - at)) for at in range(0, t, chunk)]
        start += t
    return runs


def train_epoch(net: Nnet, corpus: Corpus, pdfs, minibatch_size: int, srand: int = 0,
                chunk=None):
    """One epoch over the corpus, as nnet-shuffle-egs --srand followed by the
    nnet-train loop: one numpy permutation of all corpus rows seeded by
    `srand`, minibatches of `minibatch_size` (the remainder trained as a last,
    smaller one), labels (n, pdfs[frames[n]], 1.0).  `pdfs`: one class per
    corpus row (host).  Returns (objf, frames) of ObjfTotal(reset=True), which
    synchronises; totals accumulated before the call are included.
    With chunk=k the examples are shuffled in runs (chunk_runs: each utterance
    cut into stretches of k consecutive rows): one permutation of the runs,
    minibatches of max(1, minibatch_size // k) runs (the remainder a last one),
    each trained by PropagateFrames(share_time=True) and BackpropXent, so the
    convolutional prefix runs once per time step of a run."""
    import numpy as np
    pdfs = np.ascontiguousarray(pdfs, np.int32).ravel()
    rows = corpus.NumRows()
    if len(pdfs) != rows:
        raise KcnnError(f"train_epoch: {len(pdfs)} pdfs for a corpus of {rows} rows")
    if minibatch_size < 1:
        raise KcnnError(f"train_epoch: minibatch_size {minibatch_size}")
    if chunk is not None:
        if int(chunk) < 1:
            raise KcnnError(f"train_epoch: chunk {chunk}")
        runs = chunk_runs(corpus.lengths, int(chunk))
        order = np.random.default_rng(srand).permutation(len(runs))
        per = max(1, minibatch_size // int(chunk))
        for at in range(0, len(runs), per):
            frames = np.concatenate([np.arange(runs[j][0], runs[j][0] + runs[j][1],
                                               dtype=np.int32) for j in order[at:at + per]])
            n = len(frames)
            net.PropagateFrames(corpus, frames, share_time=True)
            net.BackpropXent((np.arange(n, dtype=np.int32), pdfs[frames],
                              np.ones(n, np.float32)))
        return net.ObjfTotal(reset=True)
    order = np.random.default_rng(srand).permutation(rows).astype(np.int32)
    for at in range(0, rows, minibatch_size):
        frames = order[at:at + minibatch_size]
        n = len(frames)
        net.PropagateFrames(corpus, frames)
        net.BackpropXent((np.arange(n, dtype=np.int32), pdfs[frames], np.ones(n, np.float32)))
    return net.ObjfTotal(reset=True)


def _device_view(addr, d: MatrixDim):
    """A torch tensor aliasing library-owned device memory (read-mostly)."""
    import torch
    if d.rows == 0 or d.cols == 0:
        return torch.empty((d.rows, d.cols), dtype=torch.float32, device="cuda")
    nbytes = ((d.rows - 1) * d.stride + d.cols) * 4

    class _Arr:
        __cuda_array_interface__ = {
            "shape": (nbytes // 4,), "typestr": "<f4", "data": (addr, False),
            "version": 2, "strides": None}

    flat = torch.as_tensor(_Arr(), device="cuda")
    return flat.as_strided((d.rows, d.cols), (d.stride, 1))
