"""Fused (shifted-)window attention for windows of 9x9 .. 14x14 tokens — host side of csrc/window_attn_large.hip.

`large_window_attention(qkv, scale, table, geometry)` computes what the Swin block of AutoFormerV2 / S3 does between the qkv
and proj linears (AutoFormerV2/model/SSS.py:205-243 around `WindowAttention.forward` :106-137): cyclic shift, window
partition, q k^T + the relative-position bias table, the -100 shift mask, softmax, P v, window reverse and the shift back.
The conventions are those of cream_amd.window_attn: the kernels take the packed (B, Hs*Ws, 3, H, 32) bf16 projection of the
unshifted map as it is and return (B, Hs*Ws, H*32) in the same token order; `geometry` = (Hs, Ws, w, shift, mask_shift).
Nothing of size N^2 per window is written: the side buffers are (B*nW, H, NP) fp32 row statistics, NP = w*w rounded up to
the 32-key tile, and the partials of the table gradient.

`usable_large_window(...)` says whether a configuration is covered: a device, bf16 (autocast), head_dim 32, 9 <= w <= 14,
1 <= H <= 32, an fp32 contiguous table, no active attention dropout.  There are no head transforms at these sizes.
`CREAM_IRPE_FUSED=0` switches this path off together with the other fused attentions.
"""
from . import _lib, _window_rows
from ._window_rows import HEAD_DIM, MAX_HEADS, padded_tokens  # noqa: F401  (public names of this module)

MIN_WINDOW = 9
MAX_WINDOW = 14

_family = _window_rows.Family("window_attn_large", _lib.WindowAttnLargeDesc, MIN_WINDOW, MAX_WINDOW)


def usable_large_window(qkv_dtype, device, head_dim, num_heads, window_size, table, dropout_p=0.0):
    """Decides from descriptors alone (no device is touched).  `dropout_p`: the ACTIVE attention dropout probability (0 in
    eval mode)."""
    return _family.usable(qkv_dtype, device, head_dim, num_heads, window_size, table, dropout_p)


def fwd_core(qkv, scale, table, geometry):
    """One forward launch: qkv (B, Hs*Ws, 3, H, 32) bf16, table ((2w-1)^2, H) fp32
    -> (out (B, Hs*Ws, H*32) bf16, lse (B*nW, H, NP) fp32 of the masked logits).  Outside autograd."""
    return _family.fwd_core(qkv, scale, table, geometry)


def bwd_core(dout, qkv, lse, scale, table, geometry, *, return_delta=False):
    """The two backward launches of fwd_core: -> (dqkv (B, Hs*Ws, 3, H, 32) bf16, d table).  Outside autograd.
    `return_delta`: also the (B*nW, H, NP) fp32 delta rows the query launch hands to the key launch (for the kernel tests)."""
    return _family.bwd_core(dout, qkv, lse, scale, table, geometry, return_delta=return_delta)


def large_window_attention(qkv, scale, table, geometry):
    """qkv (B, Hs*Ws, 3, H, 32) bf16 -> (B, Hs*Ws, H*32).  table: the fp32 relative_position_bias_table parameter itself;
    geometry = (Hs, Ws, w, shift, mask_shift).  The caller checks `usable_large_window(...)` first; what the kernels do not
    implement raises."""
    return _family.attention(qkv, scale, table, geometry)
