"""Fused head-mixing (shifted-)window attention for windows of 9x9 .. 12x12 — host side of csrc/window_attn_mix_large.hip.

`mix_large_window_attention(qkv, scale, table, geometry, proj_l, proj_w)` computes what a Mini-Swin block at window 12
(Mini-Swin-B fine-tuned to 384: swin_base_patch4_window7_224to384_minivit_sharenum2_adamw.yaml, heads 4 / 8 / 16 / 32) does
between the qkv and proj linears (MiniViT/Mini-Swin/models/swin_transformer_minivit.py:296-323 around
`WindowAttention.forward` :109-147): cyclic shift, window partition, q k^T + the relative-position bias table, the head-mixing
linear proj_l, the -100 shift mask, softmax, the second linear proj_w, P' v, window reverse and the shift back.  The conventions
are those of cream_amd.window_attn: the kernels take the packed (B, Hs*Ws, 3, H, 32) bf16 projection of the unshifted map as
it is and return (B, Hs*Ws, H*32) in the same token order; `geometry` = (Hs, Ws, w, shift, mask_shift).  Nothing of size N^2
per window is written: the side buffers are (B*nW, H, NP) fp32 row statistics, NP = w*w rounded up to the 32-key tile, and one
partial of the parameter gradients per workgroup of the backward's persistent grid.

`usable_mix_large_window(...)` says whether a configuration is covered: a device, bf16 (autocast), head_dim 32, 9 <= w <= 12,
fp32 contiguous proj_l / proj_w with bias and 1 <= H <= MAX_HEADS = 16, an fp32 contiguous table, no active attention
dropout.  32 mixed heads (the last stage of the 384 model: one window per image, two repeats) are refused by this function and
by the library's argument check alike: the exchange buffer costs 4 KB of LDS per head and the all-heads share of d table
23^2 x 32 x 4 = 68 KB, together more than a CU has; that stage stays composed.  `CREAM_IRPE_FUSED=0` switches this path off
together with the other fused attentions.

Routing by default goes by measurement (tools/bench_window_attention_mix_large.py,
profiles/NOTES_window_attention_mix_large.md): a shape (window, map height, map width, heads) is routed to these kernels only if
its fused median beat the composed median by more than the sum of the two spreads.  `ACCEPTED`: measured and passed.
`EXCLUDED`: measured and failed.  A shape in neither has not been measured and stays composed, as it was before these kernels;
`mix_large_window_attention` itself takes every covered shape, and a caller who has measured one adds it:
`window_attn_mix_large.ACCEPTED |= {(w, Hs, Ws, H)}`.  `PLAIN_ACCEPTED` / `PLAIN_EXCLUDED` are the same two sets for blocks
WITHOUT head transforms at 9 <= w <= 14 (the plain Swin-B window12_384 teacher), which go to
cream_amd.window_attn_large.large_window_attention.
"""
import ctypes
import os

import torch

from . import _lib, timing

MIN_WINDOW = 9
MAX_WINDOW = 12
MAX_HEADS = 16
HEAD_DIM = 32

# (w, Hs, Ws, H), measured with tools/bench_window_attention_mix_large.py (forward + backward of the attention half, B = 16,
# composed / fused; the lines are in profiles/NOTES_window_attention_mix_large.md).  The stages of the 384 recipe:
ACCEPTED = frozenset({
    (12, 96, 96, 4),                                    # 50.71 / 3.41 ms, 14.9 x
    (12, 48, 48, 8),                                    # 8.43 / 2.63 ms, 3.20 x
    (12, 24, 24, 16),                                   # 4.06 / 2.34 ms, 1.74 x
})                                                      # (12, 12, 12, 32) is outside the kernels' range
EXCLUDED = frozenset()
# without head transforms (window_attn_large): 5.10 / 2.50, 2.58 / 1.14, 1.50 / 0.68, 0.95 / 0.54 ms
PLAIN_ACCEPTED = frozenset({(12, 96, 96, 4), (12, 48, 48, 8), (12, 24, 24, 16), (12, 12, 12, 32)})
PLAIN_EXCLUDED = frozenset()


def routed(window_size, Hs, Ws, num_heads):
    """Whether a caller that routes by default sends this head-mixing shape to the kernels of this module."""
    shape = (window_size, Hs, Ws, num_heads)
    return shape in ACCEPTED and shape not in EXCLUDED


def routed_plain(window_size, Hs, Ws, num_heads):
    """Whether a caller that routes by default sends this shape WITHOUT head transforms to window_attn_large."""
    shape = (window_size, Hs, Ws, num_heads)
    return shape in PLAIN_ACCEPTED and shape not in PLAIN_EXCLUDED


def padded_tokens(window_size):
    """NP: the window's tokens rounded up to the 32-key tile (the last axis of lse and delta)."""
    return 32 * ((window_size * window_size + 31) // 32)


def _fp32_contig(*tensors):
    return all(t is not None and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def usable_mix_large_window(qkv_dtype, device, head_dim, num_heads, window_size, table, proj_l, proj_w, dropout_p=0.0):
    """Decides from descriptors alone (no device is touched).  `proj_l` / `proj_w`: the nn.Linear(H, H) modules of the
    current repeat; `dropout_p`: the ACTIVE attention dropout probability (0 in eval mode)."""
    if os.environ.get("CREAM_IRPE_FUSED", "1") == "0":
        return False
    if dropout_p > 0.0:
        return False
    if torch.device(device).type != "cuda" or qkv_dtype != torch.bfloat16:
        return False
    if head_dim != HEAD_DIM or not MIN_WINDOW <= window_size <= MAX_WINDOW:
        return False
    if proj_l is None or proj_w is None or not 1 <= num_heads <= MAX_HEADS:
        return False
    if not _fp32_contig(table) or tuple(table.shape) != ((2 * window_size - 1) ** 2, num_heads):
        return False
    for m in (proj_l, proj_w):
        if m.bias is None or not _fp32_contig(m.weight, m.bias) or tuple(m.weight.shape) != (num_heads, num_heads):
            return False
    return True


def _flops(B, nW, H, N, bwd):
    """Work the launches do on the padded key rows (recomputation included), for the timing regions.  32-deep products per
    (i, j) and head: forward 3 (S twice, P' v); backward 5 in the query launch (S and dP' twice, dS k) and 5 in the key launch.
    H x H mixes per (i, j): forward 3; backward 5 + 4."""
    NP = padded_tokens(int(round(N ** 0.5)))
    nprod, nmix = (10, 9) if bwd else (3, 3)
    return nprod * 2.0 * B * nW * H * NP * NP * 32 + nmix * 2.0 * B * nW * H * H * NP * NP


def _windows(geometry):
    Hs, Ws, w = geometry[:3]
    return (Hs // w) * (Ws // w)


def _desc(qkv, scale, table, geometry, mix, out, lse):
    B, L, _, H, D = qkv.shape
    Hs, Ws, w, shift, mask_shift = geometry
    d = _lib.WindowAttnMixLargeDesc()
    _lib.set_packed_qkv(d, qkv)
    d.out, d.lse = (out.data_ptr() if out is not None else None), lse.data_ptr()
    d.table = table.data_ptr()
    d.wl, d.bl, d.ww, d.bw = (t.data_ptr() for t in mix)
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = B, H, Hs, Ws, w, shift, mask_shift, D
    d.scale = scale
    return d


def fwd_core(qkv, scale, table, geometry, mix):
    """One forward launch: qkv (B, Hs*Ws, 3, H, 32) bf16, table ((2w-1)^2, H) fp32, mix = (wl, bl, ww, bw) fp32
    -> (out (B, Hs*Ws, H*32) bf16, lse (B*nW, H, NP) fp32 of the mixed, masked logits).  Outside autograd."""
    B, L, _, H, D = qkv.shape
    w = geometry[2]
    out = torch.empty((B, L, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B * _windows(geometry), H, padded_tokens(w)), dtype=torch.float32, device=qkv.device)
    d = _desc(qkv, scale, table, geometry, mix, out, lse)
    with torch.cuda.device(qkv.device), timing.region("window_attn_mix_large_fwd",
                                                      flops=_flops(B, _windows(geometry), H, w * w, False)):
        rc = _lib.load().cream_window_attn_mix_large_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_window_attn_mix_large_fwd")
    return out, lse


def bwd_core(dout, qkv, lse, scale, table, geometry, mix, *, return_delta=False):
    """The two backward launches of fwd_core: -> (dqkv (B, Hs*Ws, 3, H, 32) bf16, d table, (d wl, d bl, d ww, d bw)).
    Outside autograd.  `return_delta`: also the (B*nW, H, NP) fp32 delta rows the query launch hands to the key launch (for
    the kernel tests)."""
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
        blocks = lib.cream_window_attn_mix_large_blocks(ctypes.byref(d))
        if blocks < 0:
            _lib.check(blocks, "cream_window_attn_mix_large_blocks")
        psize = lib.cream_window_attn_mix_large_part_size(H, w)
        if psize < 0:
            _lib.check(psize, "cream_window_attn_mix_large_part_size")
        delta = torch.empty((B * _windows(geometry), H, padded_tokens(w)), dtype=torch.float32, device=dev)
        parts = torch.zeros((max(blocks, 1), psize), dtype=torch.float32, device=dev)
        d.delta, d.part, d.part_blocks = delta.data_ptr(), parts.data_ptr(), max(blocks, 1)
        with timing.region("window_attn_mix_large_bwd", flops=_flops(B, _windows(geometry), H, w * w, True)):
            rc = lib.cream_window_attn_mix_large_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "cream_window_attn_mix_large_bwd")
    p = parts.sum(0)                                # fixed order over the persistent grid
    dtab = p[:nu * H].reshape(nu, H)
    o = nu * H
    dmix = (p[o:o + H * H].reshape(H, H), p[o + 2 * H * H:o + 2 * H * H + H],
            p[o + H * H:o + 2 * H * H].reshape(H, H), p[o + 2 * H * H + H:o + 2 * H * H + 2 * H])
    if return_delta:
        return dqkv, dtab, dmix, delta
    return dqkv, dtab, dmix


class _Window(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, scale, table, geometry, wl, bl, ww, bw):
        mix = (wl, bl, ww, bw)
        out, lse = fwd_core(qkv, scale, table, geometry, mix)
        # every tensor the backward reads goes through save_for_backward (autograd's version check then sees an in-place
        # change of a parameter between forward and backward)
        ctx.save_for_backward(qkv, lse, table, *mix)
        ctx.scale, ctx.geometry = scale, geometry
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, lse, table = ctx.saved_tensors[:3]
        mix = tuple(ctx.saved_tensors[3:])
        dqkv, dtab, dmix = bwd_core(dout, qkv, lse, ctx.scale, table, ctx.geometry, mix)
        return (dqkv, None, dtab, None) + dmix


def mix_large_window_attention(qkv, scale, table, geometry, proj_l, proj_w):
    """qkv (B, Hs*Ws, 3, H, 32) bf16 -> (B, Hs*Ws, H*32).  table: the fp32 relative_position_bias_table parameter itself;
    geometry = (Hs, Ws, w, shift, mask_shift); proj_l / proj_w: the nn.Linear(H, H) modules of the current repeat (their fp32
    parameters are read, not autocast copies).  The caller checks `usable_mix_large_window(...)` first; what the kernels do
    not implement raises."""
    assert qkv.dim() == 5 and qkv.shape[2] == 3 and qkv.shape[4] == HEAD_DIM and qkv.stride(4) == 1
    geometry = tuple(int(g) for g in geometry)
    assert len(geometry) == 5 and qkv.shape[1] == geometry[0] * geometry[1]
    return _Window.apply(qkv, float(scale), table, geometry, proj_l.weight, proj_l.bias, proj_w.weight, proj_w.bias)
