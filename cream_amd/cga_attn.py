"""EfficientViT's cascaded group attention in one launch — host side of csrc/cga_attn.hip (inference only).

`CascadedGroupAttention` (EfficientViT/classification/model/efficientvit.py:104-181) runs its heads in sequence: head i projects
`feat_{i-1} + x_i` with a 1 x 1 `Conv2d_BN` into q (16), k (16) and v (d = C / h), passes q through a k_i x k_i depthwise
`Conv2d_BN` inside the window, and `softmax(scale q' k^T + ab_i) v` is both an output slice and the next head's input.  The
kernel does all of it for every window of a map: x (B, Hs, Ws, C) goes in as a strided view (channel stride 1 — a
channels-last NCHW tensor or a token tensor), windows are addressed in the kernel, and the output is `relu(cat(feats))` in token
order (B, Hs, Ws, C), ready for `proj`.

  * `usable_cga(...)` decides from descriptors alone;
  * `fold(module)` turns a module into the operand pack — `Conv2d_BN.fuse`'s formulas in fp32 while the module still holds its
    BatchNorms (eval mode), the convolutions' own weight and bias after `replace_batchnorm`.  The pack is cached on the versions
    (and storages) of every tensor it reads, so a `load_state_dict` or an in-place edit is seen;
  * `fwd_core(x, pack, w)` is the one launch.

Operand formats: projection weights bf16 (the composed path under autocast rounds them the same way), biases, depthwise taps and
the expanded attention bias fp32.  There is no backward and no fall-back in this module: what the kernel does not cover raises.
"""
import ctypes

import torch

from . import _lib, timing

KEY_DIM = 16
MAX_HEADS = 4
MAX_WINDOW = 8
GROUP_WIDTHS = (16, 32, 48, 64, 80, 96, 112)
KERNELS = (1, 3, 5, 7)

# Stage shapes (Cg, h, w) measured slower fused than composed: none so far (profiles/NOTES_efficientvit.md).
EXCLUDED = frozenset()


def usable_cga(dtype, device, C, num_heads, key_dim, d, w, kernels, Hs, Ws):
    """Decides from descriptors alone (no device is touched): a device, bf16, key_dim 16, d = C / h in GROUP_WIDTHS, 1 <= h <= 4,
    1 <= w <= 8, odd kernels up to 7, the map a multiple of the window."""
    if torch.device(device).type != "cuda" or dtype != torch.bfloat16:
        return False
    if key_dim != KEY_DIM or not 1 <= num_heads <= MAX_HEADS or C % num_heads or C // num_heads != d or d not in GROUP_WIDTHS:
        return False
    if not 1 <= w <= MAX_WINDOW or Hs < 1 or Ws < 1 or Hs % w or Ws % w:
        return False
    if len(kernels) < num_heads or any(k not in KERNELS for k in kernels[:num_heads]):
        return False
    return (d, num_heads, w) not in EXCLUDED


def flops(B, Hs, Ws, w, h, Cg, kernels):
    N = w * w
    per_head = sum(2 * N * Cg * (32 + Cg) + 2 * N * KEY_DIM * k * k + 2 * N * N * KEY_DIM + 2 * N * N * Cg for k in kernels[:h])
    return float(B * (Hs // w) * (Ws // w) * per_head)


def _conv_params(m):
    """A `Conv2d_BN` (Sequential c, bn) or its fused `Conv2d` -> the tensors its folded (weight, bias) are made of."""
    if isinstance(m, torch.nn.Conv2d):
        return (m.weight, m.bias)
    c, bn = m.c, m.bn
    return (c.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)


def _folded(m):
    """-> (weight, bias) fp32 of the eval-mode module: `Conv2d_BN.fuse`'s formulas."""
    if isinstance(m, torch.nn.Conv2d):
        return m.weight.float(), m.bias.float()
    c, bn = m.c, m.bn
    s = bn.weight.float() / (bn.running_var.float() + bn.eps) ** 0.5
    return c.weight.float() * s[:, None, None, None], bn.bias.float() - bn.running_mean.float() * s


def pack_operands(weights, biases, taps, tap_biases, ab):
    """Per-head fp32 tensors -> the kernel's operand pack: weights[i] (32 + Cg, Cg), biases[i] (32 + Cg), taps[i] (16, k_i, k_i),
    tap_biases[i] (16), ab (h, N, N)."""
    h = len(weights)
    Cg = weights[0].shape[1]
    KP = (Cg + 31) // 32 * 32
    dev = weights[0].device
    wqkv = torch.zeros((h, 32 + Cg, KP), dtype=torch.bfloat16, device=dev)
    for i, wt in enumerate(weights):
        wqkv[i, :, :Cg] = wt.reshape(32 + Cg, Cg).to(torch.bfloat16)
    return {
        "h": h, "Cg": Cg, "ks": tuple(int(t.shape[-1]) for t in taps),
        "wqkv": wqkv,
        "bqkv": torch.stack([b.float().reshape(-1) for b in biases]).contiguous(),
        "dw": torch.cat([t.float().reshape(-1) for t in taps]).contiguous(),
        "dwb": torch.stack([b.float().reshape(-1) for b in tap_biases]).contiguous(),
        "ab": ab.float().contiguous(),
    }


def fold(module):
    """The operand pack of a `CascadedGroupAttention` in eval mode, cached on the module."""
    tensors = [module.ab]
    for qkv, dw in zip(module.qkvs, module.dws):
        tensors += _conv_params(qkv) + _conv_params(dw)
    key = tuple((t._version, t.data_ptr(), t.dtype) for t in tensors)
    cached = getattr(module, "_cga_pack", None)
    if cached is None or cached[0] != key:
        with torch.no_grad(), torch.autocast(module.ab.device.type, enabled=False):
            qk = [_folded(m) for m in module.qkvs]
            dd = [_folded(m) for m in module.dws]
            pack = pack_operands([w for w, _ in qk], [b for _, b in qk], [w[:, 0] for w, _ in dd], [b for _, b in dd], module.ab)
        module._cga_pack = cached = (key, pack)
    return cached[1]


def fwd_core(x, pack, w, scale=KEY_DIM ** -0.5, relu=True):
    """One launch: x bf16 (B, Hs, Ws, C) with channel stride 1 (any batch / row / column strides that are multiples of 8) ->
    (B, Hs, Ws, C) bf16 contiguous.  Outside autograd."""
    B, Hs, Ws, C = x.shape
    h, Cg = pack["h"], pack["Cg"]
    assert x.dtype == torch.bfloat16 and x.stride(3) == 1 and C == h * Cg, (x.dtype, x.stride(), C, h, Cg)
    assert tuple(pack["ab"].shape) == (h, w * w, w * w), (pack["ab"].shape, h, w)
    out = torch.empty((B, Hs, Ws, C), dtype=torch.bfloat16, device=x.device)
    d = _lib.CgaDesc()
    d.x, (d.xsb, d.xsy, d.xsx) = x.data_ptr(), x.stride()[:3]
    d.wqkv, d.bqkv, d.dw, d.dwb, d.ab = (pack[n].data_ptr() for n in ("wqkv", "bqkv", "dw", "dwb", "ab"))
    d.out = out.data_ptr()
    d.B, d.Hs, d.Ws, d.w, d.h, d.Cg, d.relu = B, Hs, Ws, w, h, Cg, int(bool(relu))
    for i, k in enumerate(pack["ks"]):
        d.ks[i] = k
    d.scale = scale
    with torch.cuda.device(x.device), timing.region("cga_attn_fwd", flops=flops(B, Hs, Ws, w, h, Cg, pack["ks"])):
        rc = _lib.load().cream_cga_attn_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_cga_attn_fwd")
    return out
