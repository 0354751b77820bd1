"""Thin wrappers over the C ABI of csrc/pruned_ops.hip (include/cream_amd.h, "pruned TinyCLIP towers on zero-padded
operands"): rows between the compact and the padded layout, and the compact gradient finalisation.  Device tensors only; a
missing kernel is an error."""
import ctypes

import torch

from .. import _lib, timing
from ..autoformer.block import _p, _stream

GRANULE = 8          # every GEMM of the path (NT, NT + GELU, dgrad, dgrad x gelu', TN weight gradient) takes N, K, ld % 8 == 0


def padded(n):
    return -(-n // GRANULE) * GRANULE


def _dtype(t):
    if t.dtype == torch.float32:
        return _lib.F32
    if t.dtype == torch.bfloat16:
        return _lib.BF16
    raise TypeError(f"cream_amd: pad / unpad take fp32 or bf16 rows, not {t.dtype}")


def pad_cols(x2d, Dp, out=None):
    """(M, d) fp32 | bf16 contiguous -> (M, Dp) fp32, zeros in columns d .. Dp."""
    M, d = x2d.shape
    assert x2d.is_contiguous()
    if out is None:
        out = torch.empty((M, Dp), dtype=torch.float32, device=x2d.device)
    with timing.region("pad_cols", nbytes=M * (d * x2d.element_size() + Dp * 4)):
        _lib.check(_lib.load().cream_pad_cols(_p(out), _p(x2d), _dtype(x2d), M, d, Dp, _stream()), "cream_pad_cols")
    return out


def unpad_cols(x2d, d, dtype):
    """(M, Dp) fp32 -> (M, d) in `dtype` (fp32 | bf16)."""
    M, Dp = x2d.shape
    out = torch.empty((M, d), dtype=dtype, device=x2d.device)
    with timing.region("unpad_cols", nbytes=M * (d * out.element_size() + Dp * 4)):
        _lib.check(_lib.load().cream_unpad_cols(_p(out), _dtype(out), _p(x2d), M, d, Dp, _stream()), "cream_unpad_cols")
    return out


class CompactGradJobs:
    """One launch of cream_grad_finalize_compact: `add` names a parameter of compact shape (rows, cols) and the partial sums,
    laid out with row stride `ld_src` >= cols, that go into its `.grad` (created uninitialised and overwritten when the
    parameter has none)."""

    def __init__(self):
        self.jobs = (_lib.GradCompactJob * _lib.MAX_COMPACT_JOBS)()
        self.n = 0
        self.keep = []

    def add(self, param, src, nparts, pstride, rows, cols, ld_src, src_offset=0):
        assert rows * cols == param.numel()
        fresh = param.grad is None
        if fresh:
            param.grad = torch.empty_like(param, memory_format=torch.contiguous_format)
        g = param.grad
        assert g.is_contiguous() and g.dtype == torch.float32
        j = self.jobs[self.n]
        j.dst, j.src = g.data_ptr(), src.data_ptr() + src_offset * src.element_size()
        j.ld_dst, j.ld_src, j.pstride = cols, ld_src, pstride
        j.nparts, j.rows, j.cols = nparts, rows, cols
        j.src_bf16, j.overwrite = (1 if src.dtype == torch.bfloat16 else 0), (1 if fresh else 0)
        self.n += 1
        self.keep.append(src)

    def launch(self):
        with timing.region("grad_finalize_compact"):
            _lib.check(_lib.load().cream_grad_finalize_compact(ctypes.cast(self.jobs, ctypes.c_void_p), self.n, _stream()),
                       "cream_grad_finalize_compact")
        self.keep.clear()
