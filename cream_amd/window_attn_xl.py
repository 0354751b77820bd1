"""Fused window attention for windows of 15x15 .. 32x32 tokens — host side of csrc/window_attn_xl.hip.

`xl_window_attention(qkv, scale, table, geometry)` computes what a TinyViT block at high resolution does between the qkv and
proj linears (TinyViT/models/tiny_vit.py:216-286 inside :289-383; windows of 16, 24 and 32 in tiny_vit_21m_384 / _512): window
partition, q k^T + the relative-position bias table, softmax, P v, window reverse.  The conventions are those of
cream_amd.window_attn_large: the kernels take the packed (B, Hs*Ws, 3, H, 32) bf16 projection of the map as it is and return
(B, Hs*Ws, H*32) in the same token order; `geometry` = (Hs, Ws, w, shift, mask_shift) with shift = mask_shift = 0 (no model
shifts a window this large; the argument check refuses anything else).  Keys and values stream through LDS, so nothing of size
N^2 per window is written: the side buffers are (B*nW, H, NP) fp32 row statistics, NP = w*w rounded up to the 32-key tile, and
the partials of the table gradient.

`usable_xl_window(...)` says whether a configuration is covered: a device, bf16 (autocast), head_dim 32, 15 <= w <= 32,
1 <= H <= 32, an fp32 contiguous table, no active attention dropout.  `CREAM_IRPE_FUSED=0` switches this path off together
with the other fused attentions.  `ACCEPTED` holds the (w, Hs, Ws, H) shapes that were measured and beat the composed path,
`EXCLUDED` those that were measured and did not (profiles/NOTES_window_attention_xl.md); a caller that routes by default asks
`routed(...)`, so an unmeasured shape keeps the path it had.
"""
import ctypes
import os

import torch

from . import _lib, timing

MAX_HEADS = 32
MIN_WINDOW = 15
MAX_WINDOW = 32
HEAD_DIM = 32

# Routing by default goes by measurement (tools/bench_window_attention_xl.py, profiles/NOTES_window_attention_xl.md): a shape
# (window, map height, map width, heads) is routed here only if its fused median beat the composed median by more than the sum
# of the two spreads.  ACCEPTED: measured and passed.  EXCLUDED: measured and failed (none so far).  A shape in neither has not
# been measured and stays composed, as it was before these kernels; `xl_window_attention` itself takes every covered shape, and
# a caller who has measured one adds it: `window_attn_xl.ACCEPTED |= {(w, Hs, Ws, H)}`.
ACCEPTED = frozenset({
    (24, 24, 24, 12),                                   # tiny_vit_21m_384, stage 2
    (16, 64, 64, 6), (32, 32, 32, 12), (16, 16, 16, 18),  # tiny_vit_21m_512, stages 1 to 3
    (16, 32, 32, 6), (16, 32, 32, 2), (24, 24, 24, 3), (16, 16, 16, 2),   # the narrow shapes of the tests
})
EXCLUDED = frozenset()


def routed(window_size, Hs, Ws, num_heads):
    """Whether a caller that routes by default sends this shape to the kernels."""
    shape = (window_size, Hs, Ws, num_heads)
    return shape in ACCEPTED and shape not in EXCLUDED


def padded_tokens(window_size):
    """NP: the window's tokens rounded up to the 32-key tile (the last axis of lse and delta)."""
    return 32 * ((window_size * window_size + 31) // 32)


def usable_xl_window(qkv_dtype, device, head_dim, num_heads, window_size, table, dropout_p=0.0):
    """Decides from descriptors alone (no device is touched).  `dropout_p`: the ACTIVE attention dropout probability (0 in
    eval mode)."""
    if os.environ.get("CREAM_IRPE_FUSED", "1") == "0":
        return False
    if dropout_p > 0.0:
        return False
    if torch.device(device).type != "cuda" or qkv_dtype != torch.bfloat16:
        return False
    if head_dim != HEAD_DIM or not MIN_WINDOW <= window_size <= MAX_WINDOW:
        return False
    if not 1 <= num_heads <= MAX_HEADS:
        return False
    if table is None or table.dtype != torch.float32 or not table.is_contiguous():
        return False
    return tuple(table.shape) == ((2 * window_size - 1) ** 2, num_heads)


def _flops(B, nW, H, N, bwd):
    """Work the launches do on the padded key rows (recomputation included), for the timing regions.  32-deep products per
    (i, j) and head: forward 3 (S twice, P v); backward 5 in the query launch (S and dP twice, dS k) and 4 in the key launch."""
    NP = 32 * ((N + 31) // 32)
    return (9 if bwd else 3) * 2.0 * B * nW * H * NP * NP * 32


def _desc(qkv, scale, table, geometry, out, lse):
    B, L, _, H, D = qkv.shape
    Hs, Ws, w, shift, mask_shift = geometry
    d = _lib.WindowAttnXlDesc()
    _lib.set_packed_qkv(d, qkv)
    d.out, d.lse = (out.data_ptr() if out is not None else None), lse.data_ptr()
    d.table = table.data_ptr()
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = B, H, Hs, Ws, w, shift, mask_shift, D
    d.scale = scale
    return d


def _windows(geometry):
    Hs, Ws, w = geometry[:3]
    return (Hs // w) * (Ws // w)


def fwd_core(qkv, scale, table, geometry):
    """One forward launch: qkv (B, Hs*Ws, 3, H, 32) bf16, table ((2w-1)^2, H) fp32
    -> (out (B, Hs*Ws, H*32) bf16, lse (B*nW, H, NP) fp32 of the logits).  Outside autograd."""
    B, L, _, H, D = qkv.shape
    w = geometry[2]
    out = torch.empty((B, L, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B * _windows(geometry), H, padded_tokens(w)), dtype=torch.float32, device=qkv.device)
    d = _desc(qkv, scale, table, geometry, out, lse)
    with torch.cuda.device(qkv.device), timing.region("window_attn_xl_fwd", flops=_flops(B, _windows(geometry), H, w * w, False)):
        rc = _lib.load().cream_window_attn_xl_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_window_attn_xl_fwd")
    return out, lse


def bwd_core(dout, qkv, lse, scale, table, geometry, *, return_delta=False):
    """The two backward launches of fwd_core: -> (dqkv (B, Hs*Ws, 3, H, 32) bf16, d table).  Outside autograd.
    `return_delta`: also the (B*nW, H, NP) fp32 delta rows the query launch hands to the key launch (for the kernel tests)."""
    B, L, _, H, D = qkv.shape
    w = geometry[2]
    dev = qkv.device
    dout = dout.contiguous()
    dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
    d = _desc(qkv, scale, table, geometry, None, lse)
    d.dout = dout.data_ptr()
    _lib.set_packed_dqkv(d, dqkv)
    lib = _lib.load()
    nu = (2 * w - 1) ** 2
    with torch.cuda.device(dev):
        blocks = lib.cream_window_attn_xl_blocks(ctypes.byref(d))
        if blocks < 0:
            _lib.check(blocks, "cream_window_attn_xl_blocks")
        psize = lib.cream_window_attn_xl_part_size(H, w)
        if psize < 0:
            _lib.check(psize, "cream_window_attn_xl_part_size")
        delta = torch.empty((B * _windows(geometry), H, padded_tokens(w)), dtype=torch.float32, device=dev)
        parts = torch.zeros((max(blocks, 1), psize), dtype=torch.float32, device=dev)
        d.delta, d.part, d.part_blocks = delta.data_ptr(), parts.data_ptr(), max(blocks, 1)
        with timing.region("window_attn_xl_bwd", flops=_flops(B, _windows(geometry), H, w * w, True)):
            rc = lib.cream_window_attn_xl_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "cream_window_attn_xl_bwd")
    dtab = parts.sum(0).reshape(nu, H)              # fixed order over the persistent grid
    if return_delta:
        return dqkv, dtab, delta
    return dqkv, dtab


class _XlWindow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, scale, table, geometry):
        out, lse = fwd_core(qkv, scale, table, geometry)
        # every tensor the backward reads goes through save_for_backward (autograd's version check then sees an in-place
        # change of a parameter between forward and backward)
        ctx.save_for_backward(qkv, lse, table)
        ctx.scale, ctx.geometry = scale, geometry
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, lse, table = ctx.saved_tensors
        dqkv, dtab = bwd_core(dout, qkv, lse, ctx.scale, table, ctx.geometry)
        return dqkv, None, dtab, None


def xl_window_attention(qkv, scale, table, geometry):
    """qkv (B, Hs*Ws, 3, H, 32) bf16 -> (B, Hs*Ws, H*32).  table: the fp32 ((2w-1)^2, H) table; geometry = (Hs, Ws, w, 0, 0).
    The caller checks `usable_xl_window(...)` first; what the kernels do not implement raises."""
    assert qkv.dim() == 5 and qkv.shape[2] == 3 and qkv.shape[4] == HEAD_DIM and qkv.stride(4) == 1
    geometry = tuple(int(g) for g in geometry)
    assert len(geometry) == 5 and qkv.shape[1] == geometry[0] * geometry[1]
    return _XlWindow.apply(qkv, float(scale), table, geometry)
