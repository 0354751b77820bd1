"""Host side shared by the two per-head window attention families (csrc/window_attn_rows.hpp): window_attn_large (9x9 .. 14x14)
and window_attn_xl (15x15 .. 32x32).  They take the same descriptor, keep the same side buffers ((B*nW, H, NP) fp32 row
statistics and the partials of the table gradient) and differ in the C symbols, the timing regions and the window range, which
is what a `Family` holds.  The public modules instantiate one each and keep their names and documentation.
"""
import ctypes
import os

import torch

from . import _lib, timing

MAX_HEADS = 32
HEAD_DIM = 32


def padded_tokens(window_size):
    """NP: the window's tokens rounded up to the 32-key tile (the last axis of lse and delta)."""
    return 32 * ((window_size * window_size + 31) // 32)


def _windows(geometry):
    Hs, Ws, w = geometry[:3]
    return (Hs // w) * (Ws // w)


def _flops(B, nW, H, N, bwd):
    """Work the launches do on the padded key rows (recomputation included), for the timing regions.  32-deep products per
    (i, j) and head: forward 3 (S twice, P v); backward 5 in the query launch (S and dP twice, dS k) and 4 in the key launch."""
    NP = 32 * ((N + 31) // 32)
    return (9 if bwd else 3) * 2.0 * B * nW * H * NP * NP * 32


def _desc(desc_cls, qkv, scale, table, geometry, out, lse):
    B, L, _, H, D = qkv.shape
    Hs, Ws, w, shift, mask_shift = geometry
    d = desc_cls()
    _lib.set_packed_qkv(d, qkv)
    d.out, d.lse = (out.data_ptr() if out is not None else None), lse.data_ptr()
    d.table = table.data_ptr()
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = B, H, Hs, Ws, w, shift, mask_shift, D
    d.scale = scale
    return d


class _Window(torch.autograd.Function):
    @staticmethod
    def forward(ctx, family, qkv, scale, table, geometry):
        out, lse = family.fwd_core(qkv, scale, table, geometry)
        # every tensor the backward reads goes through save_for_backward (autograd's version check then sees an in-place
        # change of a parameter between forward and backward)
        ctx.save_for_backward(qkv, lse, table)
        ctx.family, ctx.scale, ctx.geometry = family, scale, geometry
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, lse, table = ctx.saved_tensors
        dqkv, dtab = ctx.family.bwd_core(dout, qkv, lse, ctx.scale, table, ctx.geometry)
        return None, dqkv, None, dtab, None


class Family:
    """One kernel family: the library calls cream_<name>_{fwd,bwd,blocks,part_size}, the timing regions <name>_fwd / _bwd,
    the descriptor class and the window sizes it covers."""

    def __init__(self, name, desc_cls, min_window, max_window):
        self.desc_cls, self.min_window, self.max_window = desc_cls, min_window, max_window
        self.region_fwd, self.region_bwd = name + "_fwd", name + "_bwd"
        self.sym_fwd, self.sym_bwd, self.sym_blocks, self.sym_part_size = (
            "cream_%s_%s" % (name, what) for what in ("fwd", "bwd", "blocks", "part_size"))

    @staticmethod
    def _count(lib, sym, *args):
        """A library call that returns a count, or a negative error code (raised)."""
        n = getattr(lib, sym)(*args)
        if n < 0:
            _lib.check(n, sym)
        return n

    def usable(self, qkv_dtype, device, head_dim, num_heads, window_size, table, dropout_p=0.0):
        if os.environ.get("CREAM_IRPE_FUSED", "1") == "0":
            return False
        if dropout_p > 0.0:
            return False
        if torch.device(device).type != "cuda" or qkv_dtype != torch.bfloat16:
            return False
        if head_dim != HEAD_DIM or not self.min_window <= window_size <= self.max_window:
            return False
        if not 1 <= num_heads <= MAX_HEADS:
            return False
        if table is None or table.dtype != torch.float32 or not table.is_contiguous():
            return False
        return tuple(table.shape) == ((2 * window_size - 1) ** 2, num_heads)

    def fwd_core(self, qkv, scale, table, geometry):
        B, L, _, H, D = qkv.shape
        w = geometry[2]
        out = torch.empty((B, L, H * D), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((B * _windows(geometry), H, padded_tokens(w)), dtype=torch.float32, device=qkv.device)
        d = _desc(self.desc_cls, qkv, scale, table, geometry, out, lse)
        with torch.cuda.device(qkv.device), timing.region(self.region_fwd, flops=_flops(B, _windows(geometry), H, w * w, False)):
            rc = getattr(_lib.load(), self.sym_fwd)(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, self.sym_fwd)
        return out, lse

    def bwd_core(self, dout, qkv, lse, scale, table, geometry, *, return_delta=False):
        B, L, _, H, D = qkv.shape
        w = geometry[2]
        dev = qkv.device
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
        d = _desc(self.desc_cls, qkv, scale, table, geometry, None, lse)
        d.dout = dout.data_ptr()
        _lib.set_packed_dqkv(d, dqkv)
        lib = _lib.load()
        nu = (2 * w - 1) ** 2
        with torch.cuda.device(dev):
            blocks = self._count(lib, self.sym_blocks, ctypes.byref(d))
            psize = self._count(lib, self.sym_part_size, H, w)
            delta = torch.empty((B * _windows(geometry), H, padded_tokens(w)), dtype=torch.float32, device=dev)
            parts = torch.zeros((max(blocks, 1), psize), dtype=torch.float32, device=dev)
            d.delta, d.part, d.part_blocks = delta.data_ptr(), parts.data_ptr(), max(blocks, 1)
            with timing.region(self.region_bwd, flops=_flops(B, _windows(geometry), H, w * w, True)):
                rc = getattr(lib, self.sym_bwd)(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, self.sym_bwd)
        dtab = parts.sum(0).reshape(nu, H)              # fixed order over the persistent grid
        if return_delta:
            return dqkv, dtab, delta
        return dqkv, dtab

    def attention(self, qkv, scale, table, geometry):
        assert qkv.dim() == 5 and qkv.shape[2] == 3 and qkv.shape[4] == HEAD_DIM and qkv.stride(4) == 1
        geometry = tuple(int(g) for g in geometry)
        assert len(geometry) == 5 and qkv.shape[1] == geometry[0] * geometry[1]
        return _Window.apply(self, qkv, float(scale), table, geometry)
