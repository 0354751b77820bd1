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
from . import _lib, _window_rows
from ._window_rows import HEAD_DIM, MAX_HEADS, padded_tokens  # noqa: F401  (public names of this module)

MIN_WINDOW = 15
MAX_WINDOW = 32

_family = _window_rows.Family("window_attn_xl", _lib.WindowAttnXlDesc, MIN_WINDOW, MAX_WINDOW)

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


def usable_xl_window(qkv_dtype, device, head_dim, num_heads, window_size, table, dropout_p=0.0):
    """Decides from descriptors alone (no device is touched).  `dropout_p`: the ACTIVE attention dropout probability (0 in
    eval mode)."""
    return _family.usable(qkv_dtype, device, head_dim, num_heads, window_size, table, dropout_p)


def fwd_core(qkv, scale, table, geometry):
    """One forward launch: qkv (B, Hs*Ws, 3, H, 32) bf16, table ((2w-1)^2, H) fp32
    -> (out (B, Hs*Ws, H*32) bf16, lse (B*nW, H, NP) fp32 of the logits).  Outside autograd."""
    return _family.fwd_core(qkv, scale, table, geometry)


def bwd_core(dout, qkv, lse, scale, table, geometry, *, return_delta=False):
    """The two backward launches of fwd_core: -> (dqkv (B, Hs*Ws, 3, H, 32) bf16, d table).  Outside autograd.
    `return_delta`: also the (B*nW, H, NP) fp32 delta rows the query launch hands to the key launch (for the kernel tests)."""
    return _family.bwd_core(dout, qkv, lse, scale, table, geometry, return_delta=return_delta)


def xl_window_attention(qkv, scale, table, geometry):
    """qkv (B, Hs*Ws, 3, H, 32) bf16 -> (B, Hs*Ws, H*32).  table: the fp32 ((2w-1)^2, H) table; geometry = (Hs, Ws, w, 0, 0).
    The caller checks `usable_xl_window(...)` first; what the kernels do not implement raises."""
    return _family.attention(qkv, scale, table, geometry)
