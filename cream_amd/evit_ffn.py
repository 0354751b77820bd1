"""EfficientViT's depthwise 3 x 3 + FFN pair and `proj` + residual on the token layout — host side of csrc/evit_ffn.hip
(inference only).

Every `EfficientViTBlock` (EfficientViT/classification/model/efficientvit.py:250-282) is dw0 -> ffn0 -> mixer -> dw1 -> ffn1,
each a `Residual`; the `Sequential`s around `PatchMerging` are the same dw -> ffn pair.  In eval mode every `Conv2d_BN` is a
convolution with a bias, so a pair is

    y1 = x + dw3x3(x)                      y2 = y1 + W2 relu(W1 y1 + b1) + b2

and ONE launch computes it on a (B, H, W, C) bf16 view with channel stride 1 (a token tensor, a slice, a channels-last NCHW
tensor): x is read once, y2 written once, y1 and the hidden activation never reach memory.

  * `usable_dwffn(...)` / `usable_pw(...)` decide from descriptors alone;
  * `fold_dwffn(dw, ffn)` / `fold_pw(conv)` turn modules into operand packs — `Conv2d_BN.fuse`'s formulas in fp32 while the
    modules still hold their BatchNorms (eval mode), the convolutions' own weight and bias after `replace_batchnorm` — cached on
    the versions (and storages) of every tensor they read, so a `load_state_dict` or an in-place edit is seen;
  * `fwd_dwffn(x, pack)` and `fwd_pw_residual(a, res, pack)` are one launch each.

Operand formats: the 1 x 1 weights bf16 (the composed path under autocast rounds them the same way), the depthwise taps and
every bias fp32.  There is no backward and no fall-back in this module: what the kernels do not cover raises.
"""
import ctypes

import torch

from . import _lib, timing
from .cga_attn import _conv_params, _folded

MAX_C, MAX_CH = 384, 768

# Pair shapes (C, Ch, H, W) and proj shapes (Cin, Cout) measured slower fused than composed: none so far
# (profiles/NOTES_efficientvit_tokens.md).
EXCLUDED = frozenset()


def usable_dwffn(dtype, device, C, Ch, H, W):
    """Decides from descriptors alone (no device is touched): a device, bf16, 16 <= C <= 384 in steps of 16, 32 <= Ch <= 768 in
    steps of 32, a map of at least one token."""
    if torch.device(device).type != "cuda" or dtype != torch.bfloat16:
        return False
    if not 16 <= C <= MAX_C or C % 16 or not 32 <= Ch <= MAX_CH or Ch % 32 or H < 1 or W < 1:
        return False
    return (C, Ch, H, W) not in EXCLUDED


def usable_pw(dtype, device, Cin, Cout):
    """Decides from descriptors alone: a device, bf16, 16 <= Cin, Cout <= 384 in steps of 16."""
    if torch.device(device).type != "cuda" or dtype != torch.bfloat16:
        return False
    if not 16 <= Cin <= MAX_C or Cin % 16 or not 16 <= Cout <= MAX_C or Cout % 16:
        return False
    return (Cin, Cout) not in EXCLUDED


def view_ok(t):
    """Does the (B, H, W, C) tensor go into the kernels as it is?  (bf16, channel stride 1, the other strides multiples of 8 and
    tokens apart, the base 16-byte aligned.)"""
    return (t.dtype == torch.bfloat16 and t.stride(3) == 1 and not any(s % 8 for s in t.stride()[:3]) and t.stride(2) >= t.shape[3]
            and t.data_ptr() % 16 == 0)


def flops_dwffn(B, H, W, C, Ch):
    return float(B * H * W) * (2 * 9 * C + 4 * C * Ch)


def flops_pw(B, H, W, Cin, Cout):
    return float(B * H * W) * 2 * Cin * Cout


def _pad_k(w):
    """(rows, K) fp32 -> bf16 (rows, K rounded up to 32), zeros past K."""
    rows, K = w.shape
    out = torch.zeros((rows, (K + 31) // 32 * 32), dtype=torch.bfloat16, device=w.device)
    out[:, :K] = w.to(torch.bfloat16)
    return out


def pack_dwffn(taps, dwb, w1, b1, w2, b2):
    """fp32 tensors -> the pair's operand pack: taps (C, 3, 3), dwb (C), w1 (Ch, C), b1 (Ch), w2 (C, Ch), b2 (C)."""
    C, Ch = w2.shape
    assert tuple(taps.shape) == (C, 3, 3) and tuple(w1.shape) == (Ch, C), (taps.shape, w1.shape, w2.shape)
    return {
        "C": C, "Ch": Ch,
        "taps": taps.float().reshape(C, 9).t().contiguous(),          # (9, C): channel fastest
        "dwb": dwb.float().reshape(C).clone(),
        "w1": _pad_k(w1.float()), "b1": b1.float().reshape(Ch).clone(),
        "w2": w2.to(torch.bfloat16).contiguous(), "b2": b2.float().reshape(C).clone(),
    }


def pack_pw(w, b):
    """fp32 w (Cout, Cin), b (Cout) -> the operand pack of `fwd_pw_residual`."""
    Cout, Cin = w.shape
    return {"Cin": Cin, "Cout": Cout, "w": _pad_k(w.float()), "b": b.float().reshape(Cout).clone()}


def _inner(m):
    """A `Residual` (or several) around a module -> the module."""
    while type(m).__name__ == "Residual":
        m = m.m
    return m


def _cached(owner, attr, tensors, make):
    key = tuple((t._version, t.data_ptr(), t.dtype) for t in tensors)
    cached = getattr(owner, attr, None)
    if cached is None or cached[0] != key:
        with torch.no_grad(), torch.autocast(tensors[0].device.type, enabled=False):
            pack = make()
        cached = (key, pack)
        setattr(owner, attr, cached)
    return cached[1]


def fold_dwffn(dw, ffn):
    """The operand pack of a depthwise 3 x 3 `Conv2d_BN` (or its fused `Conv2d`) followed by an `FFN`, each bare or inside its
    `Residual`, in eval mode; cached on the FFN."""
    dw, ffn = _inner(dw), _inner(ffn)
    tensors = list(_conv_params(dw) + _conv_params(ffn.pw1) + _conv_params(ffn.pw2))

    def make():
        (wd, bd), (w1, b1), (w2, b2) = _folded(dw), _folded(ffn.pw1), _folded(ffn.pw2)
        assert wd.shape[1:] == (1, 3, 3) and w1.shape[2:] == (1, 1) and w2.shape[2:] == (1, 1), (wd.shape, w1.shape, w2.shape)
        return pack_dwffn(wd[:, 0], bd, w1[:, :, 0, 0], b1, w2[:, :, 0, 0], b2)
    return _cached(ffn, "_evit_dwffn_pack", tensors, make)


def fold_pw(conv):
    """The operand pack of a 1 x 1 `Conv2d_BN` (or its fused `Conv2d`) in eval mode; cached on the module."""
    def make():
        w, b = _folded(conv)
        assert w.shape[2:] == (1, 1), w.shape
        return pack_pw(w[:, :, 0, 0], b)
    return _cached(conv, "_evit_pw_pack", list(_conv_params(conv)), make)


def fwd_dwffn(x, pack):
    """One launch: x bf16 (B, H, W, C) with channel stride 1 (any batch / row / column strides that are multiples of 8) ->
    (B, H, W, C) bf16 contiguous.  Outside autograd."""
    B, H, W, C = x.shape
    Ch = pack["Ch"]
    assert x.dtype == torch.bfloat16 and C == pack["C"], (x.dtype, C, pack["C"])
    if not usable_dwffn(x.dtype, x.device, C, Ch, H, W):
        raise RuntimeError(f"cream_amd.evit_ffn: the pair (C={C}, Ch={Ch}, {H} x {W}) on {x.device} is not covered")
    out = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=x.device)
    d = _lib.EvitDwffnDesc()
    d.x, (d.xsb, d.xsy, d.xsx, d.xsc) = x.data_ptr(), x.stride()
    d.taps, d.dwb, d.w1, d.b1, d.w2, d.b2 = (pack[n].data_ptr() for n in ("taps", "dwb", "w1", "b1", "w2", "b2"))
    d.out = out.data_ptr()
    d.B, d.H, d.W, d.C, d.Ch = B, H, W, C, Ch
    with torch.cuda.device(x.device), timing.region("evit_dwffn_fwd", flops=flops_dwffn(B, H, W, C, Ch)):
        rc = _lib.load().cream_evit_dwffn_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_evit_dwffn_fwd")
    return out


def fwd_pw_residual(a, res, pack):
    """One launch: out = res + W a + b.  a (B, H, W, Cin) and res (B, H, W, Cout) bf16 views under the rules of `fwd_dwffn`'s x
    -> (B, H, W, Cout) bf16 contiguous.  Outside autograd."""
    B, H, W, Cin = a.shape
    Cout = pack["Cout"]
    assert a.dtype == res.dtype == torch.bfloat16 and Cin == pack["Cin"] and tuple(res.shape) == (B, H, W, Cout), (a.shape, res.shape)
    if not usable_pw(a.dtype, a.device, Cin, Cout):
        raise RuntimeError(f"cream_amd.evit_ffn: the projection ({Cin} -> {Cout}) on {a.device} is not covered")
    out = torch.empty((B, H, W, Cout), dtype=torch.bfloat16, device=a.device)
    d = _lib.EvitPwDesc()
    d.a, (d.asb, d.asy, d.asx, d.asc) = a.data_ptr(), a.stride()
    d.res, (d.rsb, d.rsy, d.rsx, d.rsc) = res.data_ptr(), res.stride()
    d.w, d.b, d.out = pack["w"].data_ptr(), pack["b"].data_ptr(), out.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout = B, H, W, Cin, Cout
    with torch.cuda.device(a.device), timing.region("evit_pw_residual_fwd", flops=flops_pw(B, H, W, Cin, Cout)):
        rc = _lib.load().cream_evit_pw_residual_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_evit_pw_residual_fwd")
    return out
