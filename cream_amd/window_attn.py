"""Fused (shifted-)window attention of Swin / Mini-Swin — host side of csrc/window_attn.hip.

`window_attention(qkv, scale, table, geometry, proj_l, proj_w)` computes what `SwinTransformerBlock.forward_feature`
does between the qkv and proj linears (MiniViT/Mini-Swin/models/swin_transformer_minivit.py:296-323 around
`WindowAttention.forward` :109-147): cyclic shift, window partition, q k^T + the relative-position bias table, the
head-mixing linear proj_l, the -100 shift mask, softmax, the second linear proj_w, P' v, window reverse and the shift back.
qkv and proj are per-token linears, so the kernels address tokens through the window geometry instead: they take the packed
(B, Hs*Ws, 3, H, 32) bf16 projection of the unshifted map as it is and return (B, Hs*Ws, H*32) in the same token order,
ready for the proj linear.  Nothing of size N^2 per window is written: the side buffers are (B*nW, H, 64) fp32 row
statistics and one partial of the parameter gradients per workgroup of the backward's persistent grid.

`geometry` = (Hs, Ws, w, shift, mask_shift): the map, the window edge, the cyclic shift of this call (0: none) and the
shift the block's mask was built for (0: no mask).  The reference passes a block's mask whether or not the repeat rolls the
map, so the two are separate.

`usable_window(...)` says whether a configuration is covered: a device, bf16 (autocast), head_dim 32, w*w <= 64, an fp32
contiguous table, no active attention dropout, and either no head transforms with 1 <= H <= 32 or fp32 contiguous
proj_l / proj_w with 1 <= H <= MAX_HEADS_MIXED.  24 and 32 mixed heads (the 7x7 last stage of Mini-Swin-S / -B: one window
per image, two blocks) stay composed: the exchange buffer costs 4 KB of LDS per head and every head slot of a wave 32 more
accumulator registers per live tile; at 16 heads the backward already spills.  Everything else stays on the composed path
of cream_amd.miniswin.  `CREAM_IRPE_FUSED=0` switches this path off together with the other fused attentions.
"""
import ctypes
import os

import torch

from . import _lib, timing

MAX_HEADS = 32
MAX_HEADS_MIXED = 16
MAX_WINDOW_TOKENS = 64
HEAD_DIM = 32


def _fp32_contig(*tensors):
    return all(t is not None and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def usable_window(qkv_dtype, device, head_dim, num_heads, window_size, table, proj_l=None, proj_w=None, dropout_p=0.0):
    """Decides from descriptors alone (no device is touched).  `proj_l` / `proj_w`: the nn.Linear(H, H) modules of the
    current repeat or None; `dropout_p`: the ACTIVE attention dropout probability (0 in eval mode)."""
    if os.environ.get("CREAM_IRPE_FUSED", "1") == "0":
        return False
    if dropout_p > 0.0:
        return False
    if torch.device(device).type != "cuda" or qkv_dtype != torch.bfloat16:
        return False
    if head_dim != HEAD_DIM or window_size < 1 or window_size * window_size > MAX_WINDOW_TOKENS:
        return False
    if (proj_l is None) != (proj_w is None):
        return False
    if not 1 <= num_heads <= (MAX_HEADS if proj_l is None else MAX_HEADS_MIXED):
        return False
    if not _fp32_contig(table) or tuple(table.shape) != ((2 * window_size - 1) ** 2, num_heads):
        return False
    for m in (proj_l, proj_w):
        if m is not None:
            if m.bias is None or not _fp32_contig(m.weight, m.bias) or tuple(m.weight.shape) != (num_heads, num_heads):
                return False
    return True


def _flops(B, nW, H, N, mixed, bwd):
    """Work the launches do on the padded 64-key rows (recomputation included), for the timing regions.  32-deep products
    per (i, j) and head: forward 2; backward 4 in the query launch (S, dP', S again with head transforms, dS.K) and 5 in the
    key launch.  H x H mixes per (i, j): forward 2; backward 3 + 4."""
    NP = 32 * ((N + 31) // 32)
    nprod = 2 if not bwd else 9
    nmix = 0 if not mixed else (2 if not bwd else 7)
    return nprod * 2.0 * B * nW * H * NP * NP * 32 + nmix * 2.0 * B * nW * H * H * NP * NP


def _desc(qkv, scale, table, geometry, mix, out, lse):
    B, L, _, H, D = qkv.shape
    Hs, Ws, w, shift, mask_shift = geometry
    d = _lib.WindowAttnDesc()
    _lib.set_packed_qkv(d, qkv)
    d.out, d.lse = (out.data_ptr() if out is not None else None), lse.data_ptr()
    d.table = table.data_ptr()
    if mix is not None:
        d.wl, d.bl, d.ww, d.bw = (t.data_ptr() for t in mix)
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = B, H, Hs, Ws, w, shift, mask_shift, D
    d.scale = scale
    return d


def _windows(geometry):
    Hs, Ws, w = geometry[:3]
    return (Hs // w) * (Ws // w)


def fwd_core(qkv, scale, table, geometry, mix):
    """One forward launch: qkv (B, Hs*Ws, 3, H, 32) bf16, table ((2w-1)^2, H) fp32, mix = (wl, bl, ww, bw) fp32 or None
    -> (out (B, Hs*Ws, H*32) bf16, lse (B*nW, H, 64) fp32 of the mixed, masked logits).  Outside autograd."""
    B, L, _, H, D = qkv.shape
    out = torch.empty((B, L, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B * _windows(geometry), H, 64), dtype=torch.float32, device=qkv.device)
    d = _desc(qkv, scale, table, geometry, mix, out, lse)
    with torch.cuda.device(qkv.device), timing.region("window_attn_fwd",
                                                      flops=_flops(B, _windows(geometry), H, geometry[2] ** 2, mix is not None, False)):
        rc = _lib.load().cream_window_attn_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_window_attn_fwd")
    return out, lse


def bwd_core(dout, qkv, lse, scale, table, geometry, mix, *, return_delta=False):
    """The two backward launches of fwd_core: -> (dqkv (B, Hs*Ws, 3, H, 32) bf16, d table, (d wl, d bl, d ww, d bw) or
    None).  Outside autograd.  `return_delta`: also the (B*nW, H, 64) fp32 delta rows the query launch hands to the key
    launch (for the kernel tests)."""
    B, L, _, H, D = qkv.shape
    w = geometry[2]
    dev = qkv.device
    dout = dout.contiguous()
    dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
    d = _desc(qkv, scale, table, geometry, mix, None, lse)
    d.dout = dout.data_ptr()
    _lib.set_packed_dqkv(d, dqkv)
    lib = _lib.load()
    nu = (2 * w - 1) ** 2
    with torch.cuda.device(dev):
        blocks = lib.cream_window_attn_blocks(ctypes.byref(d))
        if blocks < 0:
            _lib.check(blocks, "cream_window_attn_blocks")
        psize = lib.cream_window_attn_part_size(H, w, int(mix is not None))
        delta = torch.empty((B * _windows(geometry), H, 64), dtype=torch.float32, device=dev)
        parts = torch.zeros((max(blocks, 1), psize), dtype=torch.float32, device=dev)
        d.delta, d.part, d.part_blocks = delta.data_ptr(), parts.data_ptr(), max(blocks, 1)
        with timing.region("window_attn_bwd", flops=_flops(B, _windows(geometry), H, w * w, mix is not None, True)):
            rc = lib.cream_window_attn_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "cream_window_attn_bwd")
    p = parts.sum(0)                                # fixed order over the persistent grid
    dtab = p[:nu * H].reshape(nu, H)
    dmix = None
    if mix is not None:
        o = nu * H
        dmix = (p[o:o + H * H].reshape(H, H), p[o + 2 * H * H:o + 2 * H * H + H],
                p[o + H * H:o + 2 * H * H].reshape(H, H), p[o + 2 * H * H + H:o + 2 * H * H + 2 * H])
    if return_delta:
        return dqkv, dtab, dmix, delta
    return dqkv, dtab, dmix


class _Window(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, scale, table, geometry, wl, bl, ww, bw):
        mix = None if wl is None else (wl, bl, ww, bw)
        out, lse = fwd_core(qkv, scale, table, geometry, mix)
        # every tensor the backward reads goes through save_for_backward (autograd's version check then sees an in-place
        # change of a parameter between forward and backward)
        ctx.save_for_backward(qkv, lse, table, *(mix or ()))
        ctx.scale, ctx.geometry = scale, geometry
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, lse, table = ctx.saved_tensors[:3]
        mix = tuple(ctx.saved_tensors[3:]) or None
        dqkv, dtab, dmix = bwd_core(dout, qkv, lse, ctx.scale, table, ctx.geometry, mix)
        return (dqkv, None, dtab, None) + (dmix if dmix is not None else (None, None, None, None))


def window_attention(qkv, scale, table, geometry, proj_l=None, proj_w=None):
    """qkv (B, Hs*Ws, 3, H, 32) bf16 -> (B, Hs*Ws, H*32).  table: the fp32 relative_position_bias_table parameter itself;
    geometry = (Hs, Ws, w, shift, mask_shift); proj_l / proj_w: the nn.Linear(H, H) modules of the current repeat (their
    fp32 parameters are read, not autocast copies) or None.  The caller checks `usable_window(...)` first; what the kernels
    do not implement raises."""
    assert qkv.dim() == 5 and qkv.shape[2] == 3 and qkv.shape[4] == HEAD_DIM and qkv.stride(4) == 1
    geometry = tuple(int(g) for g in geometry)
    assert len(geometry) == 5 and qkv.shape[1] == geometry[0] * geometry[1]
    mix = (None,) * 4 if proj_l is None else (proj_l.weight, proj_l.bias, proj_w.weight, proj_w.bias)
    return _Window.apply(qkv, float(scale), table, geometry, *mix)
