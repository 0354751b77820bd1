"""Depthwise 3 x 3 convolution on the token layout (B, Hs*Ws, C) — host side of csrc/token_dwconv.hip.

`token_dwconv3(x, weight, bias, (Hs, Ws))` computes what a TinyViT block does around its `local_conv`
(TinyViT/models/tiny_vit.py:374-376): `x.transpose(1, 2).reshape(B, C, H, W)`, a depthwise 3 x 3 `Conv2d` with stride 1 and
zero padding 1, `.view(B, C, L).transpose(1, 2)` — without either transpose: the channel axis is the fast one on the token
layout, so the convolution is a stencil over rows of C values, one read and one write.  `weight` is the (C, 1, 3, 3) fp32
`Conv2d` parameter itself (never an autocast copy), `bias` an optional (C) fp32 vector.  I/O is bf16 under bf16 autocast (or
for a bf16 input) and fp32 otherwise; accumulation is fp32.  The backward is two launches: dx (the same stencil, taps flipped)
and one fp32 partial of [dw | dbias] per workgroup, summed here in a fixed order — no atomics.

`token_dwconv7(x, weight, bias, (Hs, Ws), residual=False)` is the same for the depthwise 7 x 7 convolution (stride 1, zero
padding 3) of a Mini-Swin block repeat (MiniViT/Mini-Swin/models/swin_transformer_minivit.py:328-332) on csrc/token_dwconv7.hip,
with the block's `x + conv(x)` fused when `residual` is set.  It runs in the dtype of its input (bf16 or fp32) and looks at no
autocast state: Mini-Swin hands it the fp32 output of a LayerNorm.

`usable_token_conv(...)` / `usable_token_conv7(...)` say whether a convolution is covered, from descriptors alone.  There is no
fall-back inside this module: what the kernels do not implement raises.
"""
import ctypes

import torch

from . import _lib, timing

_DTYPES = {torch.bfloat16: _lib.BF16, torch.float32: _lib.F32}


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def usable_token_conv(dtype, device, C, kernel_size, stride=1, padding=1, dilation=1, groups=None):
    """Decides from descriptors alone (no device is touched): a device, bf16 or fp32 I/O, depthwise (groups == C), 3 x 3,
    stride 1, zero padding 1, no dilation, C a multiple of 8."""
    if torch.device(device).type != "cuda" or dtype not in _DTYPES:
        return False
    if C < 8 or C % 8 or groups != C:
        return False
    return (_pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)) == ((3, 3), (1, 1), (1, 1), (1, 1))


def fwd_bytes(B, L, C, itemsize, bias):
    """Bytes the forward has to move: x read once, y written once, taps and bias."""
    return 2 * B * L * C * itemsize + (9 + int(bias)) * C * 4


def bwd_bytes(B, L, C, itemsize, blocks):
    """Bytes the two backward launches have to move: dy read twice, x read once, dx written once, taps, the partials."""
    return 4 * B * L * C * itemsize + 9 * C * 4 + blocks * 10 * C * 4


def _desc(x, weight, hw):
    B, L, C = x.shape
    d = _lib.TokenDwconv3Desc()
    d.x, d.w = x.data_ptr(), weight.data_ptr()
    d.B, d.Hs, d.Ws, d.C, d.dtype = B, hw[0], hw[1], C, _DTYPES[x.dtype]
    return d


def _check(x, weight, hw):
    assert x.dim() == 3 and x.is_contiguous() and x.dtype in _DTYPES and x.shape[1] == hw[0] * hw[1], (x.shape, hw)
    assert weight.dtype == torch.float32 and weight.is_contiguous() and tuple(weight.shape) == (x.shape[2], 1, 3, 3), weight.shape


def fwd_core(x, weight, bias, hw):
    """One launch: x (B, Hs*Ws, C) bf16 | fp32 contiguous, weight (C, 1, 3, 3) fp32, bias (C) fp32 or None -> y like x.
    Outside autograd."""
    _check(x, weight, hw)
    B, L, C = x.shape
    y = torch.empty_like(x)
    d = _desc(x, weight, hw)
    d.y = y.data_ptr()
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and tuple(bias.shape) == (C,)
        d.bias = bias.data_ptr()
    with torch.cuda.device(x.device), timing.region("token_dwconv3_fwd", nbytes=fwd_bytes(B, L, C, x.element_size(), bias is not None),
                                                    flops=18.0 * B * L * C):
        rc = _lib.load().cream_token_dwconv3_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_token_dwconv3_fwd")
    return y


def bwd_core(dy, x, weight, hw):
    """The two backward launches: -> (dx like x, dw (C, 1, 3, 3) fp32, dbias (C) fp32).  Outside autograd."""
    _check(x, weight, hw)
    assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous()
    B, L, C = x.shape
    dx = torch.empty_like(x)
    d = _desc(x, weight, hw)
    d.dy, d.dx = dy.data_ptr(), dx.data_ptr()
    lib = _lib.load()
    with torch.cuda.device(x.device):
        blocks = lib.cream_token_dwconv3_blocks(ctypes.byref(d))
        if blocks < 1:
            _lib.check(blocks or -1, "cream_token_dwconv3_blocks")
        parts = torch.empty((blocks, 10 * C), dtype=torch.float32, device=x.device)      # every entry is written
        d.part, d.part_blocks = parts.data_ptr(), blocks
        with timing.region("token_dwconv3_bwd", nbytes=bwd_bytes(B, L, C, x.element_size(), blocks), flops=36.0 * B * L * C):
            rc = lib.cream_token_dwconv3_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "cream_token_dwconv3_bwd")
    p = parts.sum(0)                                # fixed order over the grid
    return dx, p[:9 * C].reshape(C, 1, 3, 3), p[9 * C:]


class _TokenDwconv3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, hw):
        y = fwd_core(x, weight, bias, hw)
        ctx.save_for_backward(x, weight)
        ctx.hw, ctx.has_bias = hw, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx, dw, db = bwd_core(dy.contiguous(), x, weight, ctx.hw)
        return dx, dw, (db if ctx.has_bias else None), None


def io_dtype(x):
    """The dtype the convolution runs in for this input: bf16 under bf16 autocast on its device (as the framework's
    convolution would), the input's own otherwise."""
    if x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
        return torch.bfloat16
    return x.dtype


def token_dwconv3(x, weight, bias, hw):
    """x (B, Hs*Ws, C) -> the depthwise 3 x 3 convolution of the (Hs, Ws) map, same layout, in `io_dtype(x)`.  The caller
    checks `usable_token_conv(...)` first."""
    hw = (int(hw[0]), int(hw[1]))
    x = x.to(io_dtype(x)).contiguous()
    return _TokenDwconv3.apply(x, weight, bias, hw)


# ---- 7 x 7, residual fused (csrc/token_dwconv7.hip) ------------------------------------------------------------------------------
def usable_token_conv7(dtype, device, C, kernel_size, stride=1, padding=3, dilation=1, groups=None):
    """Decides from descriptors alone (no device is touched): a device, bf16 or fp32 I/O, depthwise (groups == C), 7 x 7,
    stride 1, zero padding 3, no dilation, C a multiple of 8."""
    if torch.device(device).type != "cuda" or dtype not in _DTYPES:
        return False
    if C < 8 or C % 8 or groups != C:
        return False
    return (_pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)) == ((7, 7), (1, 1), (3, 3), (1, 1))


def fwd_bytes7(B, L, C, itemsize, bias):
    """Bytes the 7 x 7 forward has to move: x read once, y written once, taps and bias."""
    return 2 * B * L * C * itemsize + (49 + int(bias)) * C * 4


def bwd_bytes7(B, L, C, itemsize, blocks):
    """Bytes the two 7 x 7 backward launches have to move: dy read twice, x read once, dx written once, taps, the partials."""
    return 4 * B * L * C * itemsize + 49 * C * 4 + blocks * 50 * C * 4


def _desc7(x, weight, hw, residual):
    B, L, C = x.shape
    d = _lib.TokenDwconv7Desc()
    d.x, d.w = x.data_ptr(), weight.data_ptr()
    d.B, d.Hs, d.Ws, d.C, d.dtype, d.residual = B, hw[0], hw[1], C, _DTYPES[x.dtype], int(bool(residual))
    return d


def _check7(x, weight, hw):
    assert x.dim() == 3 and x.is_contiguous() and x.dtype in _DTYPES and x.shape[1] == hw[0] * hw[1], (x.shape, hw)
    assert weight.dtype == torch.float32 and weight.is_contiguous() and tuple(weight.shape) == (x.shape[2], 1, 7, 7), weight.shape


def fwd_core7(x, weight, bias, hw, residual=False):
    """One launch: x (B, Hs*Ws, C) bf16 | fp32 contiguous, weight (C, 1, 7, 7) fp32, bias (C) fp32 or None -> y like x
    (+ x with `residual`).  Outside autograd."""
    _check7(x, weight, hw)
    B, L, C = x.shape
    y = torch.empty_like(x)
    d = _desc7(x, weight, hw, residual)
    d.y = y.data_ptr()
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and tuple(bias.shape) == (C,)
        d.bias = bias.data_ptr()
    with torch.cuda.device(x.device), timing.region("token_dwconv7_fwd", nbytes=fwd_bytes7(B, L, C, x.element_size(), bias is not None),
                                                    flops=98.0 * B * L * C):
        rc = _lib.load().cream_token_dwconv7_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_token_dwconv7_fwd")
    return y


def bwd_core7(dy, x, weight, hw, residual=False):
    """The two backward launches: -> (dx like x (+ dy with `residual`), dw (C, 1, 7, 7) fp32, dbias (C) fp32).  Outside
    autograd."""
    _check7(x, weight, hw)
    assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous()
    B, L, C = x.shape
    dx = torch.empty_like(x)
    d = _desc7(x, weight, hw, residual)
    d.dy, d.dx = dy.data_ptr(), dx.data_ptr()
    lib = _lib.load()
    with torch.cuda.device(x.device):
        blocks = lib.cream_token_dwconv7_blocks(ctypes.byref(d))
        if blocks < 1:
            _lib.check(blocks or -1, "cream_token_dwconv7_blocks")
        parts = torch.empty((blocks, 50 * C), dtype=torch.float32, device=x.device)      # every entry is written
        d.part, d.part_blocks = parts.data_ptr(), blocks
        with timing.region("token_dwconv7_bwd", nbytes=bwd_bytes7(B, L, C, x.element_size(), blocks), flops=196.0 * B * L * C):
            rc = lib.cream_token_dwconv7_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "cream_token_dwconv7_bwd")
    p = parts.sum(0)                                # fixed order over the grid
    return dx, p[:49 * C].reshape(C, 1, 7, 7), p[49 * C:]


class _TokenDwconv7(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, hw, residual):
        y = fwd_core7(x, weight, bias, hw, residual)
        ctx.save_for_backward(x, weight)
        ctx.hw, ctx.has_bias, ctx.residual = hw, bias is not None, residual
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx, dw, db = bwd_core7(dy.contiguous(), x, weight, ctx.hw, ctx.residual)
        return dx, dw, (db if ctx.has_bias else None), None, None


def token_dwconv7(x, weight, bias, hw, residual=False):
    """x (B, Hs*Ws, C) bf16 | fp32 -> the depthwise 7 x 7 convolution of the (Hs, Ws) map (+ x with `residual`), same layout and
    dtype; taps and bias are the fp32 parameters themselves.  The caller checks `usable_token_conv7(...)` first."""
    hw = (int(hw[0]), int(hw[1]))
    return _TokenDwconv7.apply(x.contiguous(), weight, bias, hw, bool(residual))
