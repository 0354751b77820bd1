"""Fused Mini-DeiT attention with head transforms (conv_l before the softmax, conv_w after it) — host side of
csrc/mini_attn.hip.

`attention_mixed(qkv, scale, rpe_k, conv_l_weight, conv_w_weight)` computes what `MiniAttention.forward` does between
the qkv and proj linears when `use_transform` is on (MiniViT/Mini-DeiT/mini_vision_transformer.py:84-114): q k^T with
the contextual rpe on k, the 1x1 convolution over heads, softmax, the second convolution, P' v — without writing anything
of size L^2: the side buffers are (B, H, L) fp32 row statistics, (B, H, NP, 64) bf16 lookup / bucket-gradient rows and one
(H, H) partial of each convolution's gradient per workgroup.  It takes the packed (B, L, 3, H, 64) bf16 projection as it is
and returns (B, L, H*64) ready for the proj linear.

`usable_mixed(...)` says whether a configuration is covered: a device, bf16 (autocast), head_dim 64, 1 <= H <= 12,
L <= 2048, rpe on k only (an iRPE in contextual mode with at most 64 buckets and an fp32 contiguous table) or no rpe at
all, fp32 convolution weights, no active attention dropout.  Everything else stays on the composed path of
cream_amd.minivit.  `CREAM_IRPE_FUSED=0` switches this path off together with the other fused attentions.
"""
import ctypes
import os

import torch

from . import _lib, timing
from .irpe_fused import _term, padded_len

MAX_HEADS = 12
MAX_NB = 64


def usable_mixed(qkv_dtype, device, head_dim, num_heads, L, rpes, conv_l_weight, conv_w_weight, dropout_p=0.0):
    """Decides from descriptors alone (no device is touched).  `rpes` = (rpe_q, rpe_k, rpe_v) modules or None;
    `dropout_p`: the ACTIVE attention dropout probability (0 in eval mode)."""
    if os.environ.get("CREAM_IRPE_FUSED", "1") == "0":
        return False
    if dropout_p > 0.0:
        return False
    if torch.device(device).type != "cuda" or qkv_dtype != torch.bfloat16:
        return False
    if head_dim != 64 or not 1 <= num_heads <= MAX_HEADS or not 1 <= L <= 2048:
        return False
    for w in (conv_l_weight, conv_w_weight):
        if w is None or w.dtype != torch.float32 or tuple(w.shape) != (num_heads, num_heads, 1, 1) or not w.is_contiguous():
            return False
    rq, rk, rv = rpes
    if rq is not None or rv is not None:
        return False
    if rk is not None:
        from .irpe import iRPE
        if type(rk) is not iRPE or rk.mode != "contextual" or rk.num_buckets > MAX_NB:
            return False
        w = rk.lookup_table_weight
        if w.dtype != torch.float32 or not w.is_contiguous():
            return False
    return True


def _flops(B, H, L, bwd):
    """Work the launches do (recomputation included), for the timing regions.  64-deep products per (i, j) and head:
    forward 3 (S in both key passes, P'V); backward 2 in the delta launch (S, dP'), 2 in each of the ceil(H / 4) dq
    launches plus one dS.K for the slot's heads (counted once over all slots), 5 in the dk / dv launch.  H x H mixes per
    (i, j): forward 3; backward 2 + 3 per dq launch + 4."""
    slots = (H + 3) // 4
    nprod = 3 if not bwd else 2 + 2 * slots + 1 + 5
    nmix = 3 if not bwd else 2 + 3 * slots + 4
    return nprod * 2.0 * B * H * L * L * 64 + nmix * 2.0 * B * H * H * L * L


def _desc(qkv, scale, term, wl, ww, out, lse):
    B, L, _, H, D = qkv.shape
    d = _lib.MiniAttnDesc()
    _lib.set_packed_qkv(d, qkv)
    d.out, d.lse = (out.data_ptr() if out is not None else None), lse.data_ptr()
    nb = 1
    if term is not None:
        d.wk, d.wk_hs, d.idk, d.idk_t, nb = term[0].data_ptr(), term[1], term[2].data_ptr(), term[3].data_ptr(), term[4]
    d.wl, d.ww = wl.data_ptr(), ww.data_ptr()
    d.B, d.H, d.L, d.NP, d.nb, d.head_dim = B, H, L, padded_len(L), nb, D
    d.scale = scale
    return d


def fwd_core(qkv, scale, term, wl, ww):
    """One forward launch: qkv (B, L, 3, H, 64) bf16, term = irpe_fused._term(rpe_k) or None, wl / ww (H, H, 1, 1) fp32
    -> (out (B, L, H*64) bf16, lse (B, H, L) fp32 of the mixed logits).  Outside autograd."""
    B, L, _, H, D = qkv.shape
    out = torch.empty((B, L, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
    d = _desc(qkv, scale, term, wl, ww, out, lse)
    with torch.cuda.device(qkv.device), timing.region("mini_attn_fwd", flops=_flops(B, H, L, False)):
        rc = _lib.load().cream_mini_attn_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_mini_attn_fwd")
    return out, lse


def bwd_core(dout, qkv, lse, scale, term, wl, ww, *, return_delta=False):
    """The backward launches of fwd_core: -> (dqkv (B, L, 3, H, 64) bf16, d table or None, d wl, d ww).  Outside autograd.
    `return_delta`: also the (B, H, NP) fp32 delta rows of the first launch (for the kernel tests)."""
    B, L, _, H, D = qkv.shape
    NP = padded_len(L)
    dev = qkv.device
    dout = dout.contiguous()
    dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
    d = _desc(qkv, scale, term, wl, ww, None, lse)
    d.dout = dout.data_ptr()
    _lib.set_packed_dqkv(d, dqkv)
    delta = torch.empty((B, H, NP), dtype=torch.float32, device=dev)
    parts = torch.empty((2, B * (NP // 32), H, H), dtype=torch.float32, device=dev)
    d.delta, d.dwl_part, d.dww_part = delta.data_ptr(), parts[0].data_ptr(), parts[1].data_ptr()
    lkg = dlk = None
    if term is not None:
        lkg = torch.empty((B, H, NP, 64), dtype=qkv.dtype, device=dev)
        dlk = torch.empty((B, H, NP, 64), dtype=qkv.dtype, device=dev)
        d.lkg, d.dlk = lkg.data_ptr(), dlk.data_ptr()
    lib = _lib.load()
    dtab = None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        with timing.region("mini_attn_bwd", flops=_flops(B, H, L, True)):
            rc = lib.cream_mini_attn_bwd(ctypes.byref(d), stream)
        _lib.check(rc, "cream_mini_attn_bwd")
        if term is not None:                        # d lookup_table_weight (H', 64, nb) = (scale q)^T dlk, partials then .sum(0)
            qs = qkv.stride()
            part = torch.empty((B, H, 64, 64), dtype=torch.float32, device=dev)
            _lib.check(lib.cream_irpe_table_grad(part.data_ptr(), qkv.data_ptr(), qs[0], qs[1], qs[3], dlk.data_ptr(),
                                                 H * NP * 64, 64, NP * 64, B, H, L, scale, stream), "cream_irpe_table_grad")
            w, nb = term[0], term[4]
            g = part.sum(0)
            if w.shape[0] == 1:
                g = g.sum(0, keepdim=True)
            dtab = g[:, :, :nb].to(w.dtype).contiguous()
    dw = parts.sum(1)                               # fixed order: (2, H, H)
    res = (dqkv, dtab, dw[0].reshape(wl.shape).contiguous(), dw[1].reshape(ww.shape).contiguous())
    return res + (delta,) if return_delta else res


class _Mixed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, scale, wk, wl, ww, term):
        out, lse = fwd_core(qkv, scale, term, wl, ww)
        # every tensor the backward reads goes through save_for_backward (autograd's version check then sees an in-place
        # change of the table); the byte id matrices are constants of the table geometry, cached in irpe_fused
        ctx.save_for_backward(qkv, lse, wl, ww, *(() if term is None else (wk, term[2], term[3])))
        ctx.scale, ctx.meta = scale, (None if term is None else (term[1], term[4], term[5]))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, lse, wl, ww = ctx.saved_tensors[:4]
        term = None
        if ctx.meta is not None:
            wk, asis, tr = ctx.saved_tensors[4:]
            term = (wk, ctx.meta[0], asis, tr, ctx.meta[1], ctx.meta[2])
        dqkv, dtab, dwl, dww = bwd_core(dout, qkv, lse, ctx.scale, term, wl, ww)
        return dqkv, None, dtab, dwl, dww, None


def attention_mixed(qkv, scale, rpe_k, conv_l_weight, conv_w_weight):
    """qkv (B, L, 3, H, 64) bf16 -> (B, L, H*64).  rpe_k: the iRPE module of the current repeat or None; the two
    convolution weights are the fp32 parameters themselves ((H, H, 1, 1), not autocast copies).  The caller checks
    `usable_mixed(...)` first; what the kernels do not implement raises."""
    assert qkv.dim() == 5 and qkv.shape[2] == 3 and qkv.shape[4] == 64 and qkv.stride(4) == 1
    term = _term(rpe_k, qkv.shape[1], qkv.device)
    wk = term[0] if term is not None else None
    return _Mixed.apply(qkv, float(scale), wk, conv_l_weight, conv_w_weight, term)
