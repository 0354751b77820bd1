"""Thin wrappers over the C ABI of csrc/l0_mask.hip (include/cream_amd.h, "TinyCLIP's pruning masks folded into the
operands"): the masked LayerNorm passes, the masked operand pack and the masked gradient finalisation.  Device tensors
only; a missing kernel is an error."""
import ctypes

import torch

from .. import _lib, timing
from ..autoformer.block import _p, _stream


class HiddenMask:
    """hidden_z of a tower as the masked LayerNorm kernels take it: the fp32 mask and the number of kept columns (counted
    once per forward: one host synchronisation per tower, as the composed path's torch.where has per LayerNorm)."""
    __slots__ = ("z", "n_keep")

    def __init__(self, z):
        self.z = z.detach().contiguous()
        self.n_keep = int(torch.count_nonzero(self.z))
        if self.n_keep == 0:
            raise ValueError("hidden_z drops every column: nothing is left to normalise")


def ln_fwd_masked(x2d, gamma, beta, eps, hm):
    M, E = x2d.shape
    y = torch.empty((M, E), dtype=torch.bfloat16, device=x2d.device)
    mean = torch.empty(M, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x2d.device)
    with timing.region("ln_fwd_masked", nbytes=M * E * 6):
        _lib.check(_lib.load().cream_ln_fwd_masked(_p(y), _p(mean), _p(rstd), _p(x2d), _p(gamma), _p(beta), _p(hm.z), hm.n_keep,
                                                  M, E, float(eps), _stream()), "cream_ln_fwd_masked")
    return y, mean, rstd


def add_ln_fwd_masked(x2d, res, sample_scale, rows_per_sample, gamma, beta, eps, hm):
    """-> (x1 = x + s_b * res, y = masked LN(x1), mean, rstd)"""
    M, E = x2d.shape
    x1 = torch.empty_like(x2d)
    y = torch.empty((M, E), dtype=torch.bfloat16, device=x2d.device)
    mean = torch.empty(M, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x2d.device)
    with timing.region("ln_fwd_masked", nbytes=M * E * (4 + 2 + 4 + 2)):
        _lib.check(_lib.load().cream_add_ln_fwd_masked(_p(x1), _p(y), _p(mean), _p(rstd), _p(x2d), _p(res), _p(sample_scale),
                                                      rows_per_sample, _p(gamma), _p(beta), _p(hm.z), hm.n_keep, M, E, float(eps),
                                                      _stream()), "cream_add_ln_fwd_masked")
    return x1, y, mean, rstd


def ln_bwd_masked_raw(dy, x2d, mean, rstd, gamma, hm, dres, sample_scale, rows_per_sample, want_scaled):
    """-> (dx, dx_scaled or None, partial (P, 3, E)) — the layout of block.ln_bwd_raw."""
    M, E = x2d.shape
    lib = _lib.load()
    dx = torch.empty((M, E), dtype=torch.float32, device=x2d.device)
    dxs = torch.empty((M, E), dtype=torch.bfloat16, device=x2d.device) if want_scaled else None
    partial = torch.empty((lib.cream_ln_partials(), 3, E), dtype=torch.float32, device=x2d.device)
    with timing.region("ln_bwd_masked", nbytes=M * E * (2 + 4 + 4 + 4 + (2 if want_scaled else 0))):
        _lib.check(lib.cream_ln_bwd_masked(_p(dx), _p(dxs), _p(partial), _p(dy), _p(x2d), _p(mean), _p(rstd), _p(gamma), _p(hm.z),
                                           hm.n_keep, _p(dres), _p(sample_scale), rows_per_sample, M, E, _stream()),
                   "cream_ln_bwd_masked")
    return dx, dxs, partial


def _ptr(t):
    return t.data_ptr() if t is not None else 0


class MaskPack:
    """One launch of cream_mask_pack: `add` names an fp32 tensor viewed as (rows, cols), its masks and its bf16 copies."""

    def __init__(self):
        self.jobs = (_lib.MaskPackJob * _lib.MAX_MASK_JOBS)()
        self.n = 0
        self.nbytes = 0
        self.keep = []

    def add(self, w, r=None, c=None, c_group=1, mir=None, mir_t=None):
        assert w.is_contiguous() and w.dtype == torch.float32
        cols = w.shape[-1]
        rows = w.numel() // cols
        j = self.jobs[self.n]
        j.w, j.r, j.c, j.mir, j.mir_t = w.data_ptr(), _ptr(r), _ptr(c), _ptr(mir), _ptr(mir_t)
        j.ld, j.ld_mir, j.ld_mir_t = cols, (mir.stride(-2) if mir is not None and mir.dim() >= 2 else cols), \
            (mir_t.stride(-2) if mir_t is not None else 0)
        j.rows, j.cols, j.c_group = rows, cols, c_group
        self.n += 1
        self.nbytes += rows * cols * (4 + 2 * (mir is not None) + 2 * (mir_t is not None))
        self.keep.append((w, r, c, mir, mir_t))

    def launch(self):
        with timing.region("mask_pack", nbytes=self.nbytes):
            _lib.check(_lib.load().cream_mask_pack(ctypes.cast(self.jobs, ctypes.c_void_p), self.n, _stream()), "cream_mask_pack")
        self.keep.clear()


class MaskGradJobs:
    """One call of cream_mask_grad_finalize (two launches).  `add`: the gradient `dst` of the fp32 tensor `w` (rows, cols) from the
    partial sums of the gradient of diag(r) w diag(c); `dr_out` / `dc_out` receive the masks' gradients."""

    def __init__(self):
        self.jobs = (_lib.MaskGradJob * _lib.MAX_MASK_JOBS)()
        self.n = 0
        self.nbytes = 0
        self.keep = []

    def add(self, dst, src, nparts, pstride, w, r=None, c=None, c_group=1, dr_out=None, dc_out=None, overwrite=False, src_offset=0,
            dr_accumulate=False, dc_accumulate=False):
        cols = w.shape[-1]
        rows = w.numel() // cols
        ws = None
        if dr_out is not None or dc_out is not None:
            ws = torch.empty(_lib.load().cream_mask_grad_ws_floats(rows, cols), dtype=torch.float32, device=w.device)
        j = self.jobs[self.n]
        j.dst, j.src, j.w = dst.data_ptr(), src.data_ptr() + src_offset * src.element_size(), w.data_ptr()
        j.r, j.c, j.dr_out, j.dc_out, j.ws = _ptr(r), _ptr(c), _ptr(dr_out), _ptr(dc_out), _ptr(ws)
        j.ld, j.pstride, j.ld_w = cols, pstride, cols
        j.nparts, j.rows, j.cols, j.c_group = nparts, rows, cols, c_group
        j.src_bf16 = 1 if src.dtype == torch.bfloat16 else 0
        j.overwrite, j.dr_accumulate, j.dc_accumulate = int(overwrite), int(dr_accumulate), int(dc_accumulate)
        self.n += 1
        self.nbytes += rows * cols * (nparts * src.element_size() + 4 + (4 if overwrite else 8))
        self.keep.append((dst, src, w, r, c, dr_out, dc_out, ws))

    def launch(self):
        with timing.region("mask_grad_finalize", nbytes=self.nbytes):
            _lib.check(_lib.load().cream_mask_grad_finalize(ctypes.cast(self.jobs, ctypes.c_void_p), self.n, _stream()),
                       "cream_mask_grad_finalize")
        self.keep.clear()
