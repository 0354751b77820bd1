"""EfficientViT — host-side mirror of EfficientViT/classification/model/efficientvit.py (`Conv2d_BN` :13-34, `BN_Linear` :37-60,
`PatchMerging` :63-75, `Residual` :78-89, `FFN` :92-101, `CascadedGroupAttention` :104-181, `LocalWindowAttention` :184-247,
`EfficientViTBlock` :250-282, `EfficientViT` :285-356) and model/build.py (the six configurations :10-68, the factories :71-171,
`replace_batchnorm` :173-180) on the fused cascaded group attention of cream_amd.cga_attn.

Same constructor arguments, module nesting, parameter and buffer names as the reference, before and after `replace_batchnorm`
(`blocks2.0.0.m.c.weight`, `blocks2.1.se.fc1.weight`, `blocks2.3.mixer.m.attn.qkvs.0.bn.running_mean`, ...;
`attention_bias_idxs` is persistent here as it is there), so the published state dicts load.  Nothing here downloads:
`pretrained=True` raises.  `load_checkpoint_state_dict` keeps the factories' rule that unsqueezes 2-d checkpoint weights into
1 x 1 convolutions.

No timm: `SqueezeExcite` is written out as timm 0.5.4's `SEModule`, the release classification/requirements.txt pins — `fc1`
and `fc2` 1 x 1 convolutions with bias, mean over H and W -> fc1 -> ReLU -> fc2 -> sigmoid gate, reduced width
`make_divisible(channels * rd_ratio, 8, round_limit=0.)`.  That definition is written from memory of that release and could not
be checked against an installed timm.  Every published model has 4 dim * 0.25 = dim channels there, a multiple of 8, so the
rounding rule never acts on them.

Two paths through `LocalWindowAttention.forward`:
  * fused — a device tensor under bf16 autocast, eval mode, nothing requiring a gradient (`torch.no_grad()` or no tensor with
    `requires_grad`), `CREAM_IRPE_FUSED` not 0, `fused_attention` set, the map a multiple of the window (the reference would not
    pad) and `cga_attn.usable_cga`: x goes in as a (B, H, W, C) view, ONE launch computes every window's cascade up to the ReLU
    in front of `proj`, and `proj`'s Conv2d_BN (or its fused Conv2d) runs on the result.  No chunk, split, partition or reverse.
  * composed — everything else (training mode, fp32, the CPU, padded maps, out-of-range shapes): the reference's arithmetic
    step by step, with autograd through plain modules.  Training is out of scope for the kernel: a BatchNorm sits between every
    head's projection and its attention and needs batch statistics over all windows.

Two paths through `EfficientViT.forward`:
  * tokens — `fused_blocks` set, `CREAM_IRPE_FUSED` not 0, eval mode, a device tensor under bf16 autocast, nothing requiring a
    gradient: `patch_embed`'s output is brought to (B, H, W, C) bf16 once and stays there up to the pooling.  Every depthwise
    3 x 3 + FFN pair (two per block, one on either side of a `PatchMerging`) is ONE launch of cream_amd.evit_ffn, the mixer is
    the cascaded group attention launch followed by `proj` + residual in one launch; `PatchMerging` runs with the framework on
    the channels-last view of the token tensor.  A pair or a mixer the kernels do not cover runs composed on the view.
  * composed — everything else: the modules one after the other on NCHW, as the reference does.
The stem, `PatchMerging`, BatchNorm in training mode and the classifier stay with the framework.
"""
import itertools
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import cga_attn, evit_ffn


def _trunc_normal(t, std=.02):
    return nn.init.trunc_normal_(t, std=std, a=-2., b=2.)


def make_divisible(v, divisor=8, min_value=None, round_limit=.9):
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:
        new_v += divisor
    return new_v


class SqueezeExcite(nn.Module):
    """timm 0.5.4 `SEModule` with its defaults (see the module docstring)."""

    def __init__(self, channels, rd_ratio=1. / 16, rd_channels=None, rd_divisor=8):
        super().__init__()
        if not rd_channels:
            rd_channels = make_divisible(channels * rd_ratio, rd_divisor, round_limit=0.)
        self.fc1 = nn.Conv2d(channels, rd_channels, kernel_size=1, bias=True)
        self.bn = nn.Identity()
        self.act = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(rd_channels, channels, kernel_size=1, bias=True)
        self.gate = nn.Sigmoid()

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        s = self.fc2(self.act(self.bn(self.fc1(s))))
        return x * self.gate(s)


class Conv2d_BN(nn.Sequential):
    """:13-34."""

    def __init__(self, a, b, ks=1, stride=1, pad=0, dilation=1, groups=1, bn_weight_init=1, resolution=-10000):
        super().__init__()
        self.add_module('c', nn.Conv2d(a, b, ks, stride, pad, dilation, groups, bias=False))
        bn = nn.BatchNorm2d(b)
        nn.init.constant_(bn.weight, bn_weight_init)
        nn.init.constant_(bn.bias, 0)
        self.add_module('bn', bn)

    @torch.no_grad()
    def fuse(self):
        c, bn = self._modules.values()
        s = bn.weight / (bn.running_var + bn.eps) ** 0.5
        w = c.weight * s[:, None, None, None]
        b = bn.bias - bn.running_mean * bn.weight / (bn.running_var + bn.eps) ** 0.5
        m = nn.Conv2d(w.size(1) * c.groups, w.size(0), w.shape[2:], stride=c.stride, padding=c.padding, dilation=c.dilation,
                      groups=c.groups, device=w.device)
        m.weight.data.copy_(w)
        m.bias.data.copy_(b)
        return m


class BN_Linear(nn.Sequential):
    """:37-60."""

    def __init__(self, a, b, bias=True, std=0.02):
        super().__init__()
        self.add_module('bn', nn.BatchNorm1d(a))
        self.add_module('l', nn.Linear(a, b, bias=bias))
        _trunc_normal(self.l.weight, std=std)
        if bias:
            nn.init.constant_(self.l.bias, 0)

    @torch.no_grad()
    def fuse(self):
        bn, l = self._modules.values()
        s = bn.weight / (bn.running_var + bn.eps) ** 0.5
        b = bn.bias - bn.running_mean * bn.weight / (bn.running_var + bn.eps) ** 0.5
        w = l.weight * s[None, :]
        if l.bias is None:
            b = b @ l.weight.T
        else:
            b = (l.weight @ b[:, None]).view(-1) + l.bias
        m = nn.Linear(w.size(1), w.size(0), device=w.device)
        m.weight.data.copy_(w)
        m.bias.data.copy_(b)
        return m


class PatchMerging(nn.Module):
    """:63-75."""

    def __init__(self, dim, out_dim, input_resolution):
        super().__init__()
        hid_dim = int(dim * 4)
        self.conv1 = Conv2d_BN(dim, hid_dim, 1, 1, 0, resolution=input_resolution)
        self.act = nn.ReLU()
        self.conv2 = Conv2d_BN(hid_dim, hid_dim, 3, 2, 1, groups=hid_dim, resolution=input_resolution)
        self.se = SqueezeExcite(hid_dim, .25)
        self.conv3 = Conv2d_BN(hid_dim, out_dim, 1, 1, 0, resolution=input_resolution // 2)

    def forward(self, x):
        x = self.act(self.conv2(self.act(self.conv1(x))))
        return self.conv3(self.se(x))


class Residual(nn.Module):
    """:78-89.  The drop rule: in training mode a whole sample's branch is dropped with probability `drop`, the kept ones scaled
    by 1 / (1 - drop)."""

    def __init__(self, m, drop=0.):
        super().__init__()
        self.m = m
        self.drop = drop

    def forward(self, x):
        if self.training and self.drop > 0:
            keep = torch.rand(x.size(0), 1, 1, 1, device=x.device).ge_(self.drop).div(1 - self.drop).detach()
            return x + self.m(x) * keep
        return x + self.m(x)


class FFN(nn.Module):
    """:92-101."""

    def __init__(self, ed, h, resolution):
        super().__init__()
        self.pw1 = Conv2d_BN(ed, h, resolution=resolution)
        self.act = nn.ReLU()
        self.pw2 = Conv2d_BN(h, ed, bn_weight_init=0, resolution=resolution)

    def forward(self, x):
        return self.pw2(self.act(self.pw1(x)))


class CascadedGroupAttention(nn.Module):
    """:104-181.  `forward` is the composed path on (windows, C, w, w); the fused one is `LocalWindowAttention.forward_fused`."""

    def __init__(self, dim, key_dim, num_heads=8, attn_ratio=4, resolution=14, kernels=[5, 5, 5, 5]):
        super().__init__()
        self.num_heads = num_heads
        self.scale = key_dim ** -0.5
        self.key_dim = key_dim
        self.d = int(attn_ratio * key_dim)
        self.attn_ratio = attn_ratio
        self.kernels = tuple(kernels[:num_heads])
        self.qkvs = nn.ModuleList(Conv2d_BN(dim // num_heads, key_dim * 2 + self.d, resolution=resolution)
                                  for _ in range(num_heads))
        self.dws = nn.ModuleList(Conv2d_BN(key_dim, key_dim, kernels[i], 1, kernels[i] // 2, groups=key_dim, resolution=resolution)
                                 for i in range(num_heads))
        self.proj = nn.Sequential(nn.ReLU(), Conv2d_BN(self.d * num_heads, dim, bn_weight_init=0, resolution=resolution))
        # the reference numbers the offsets (|dy|, |dx|) in the order it meets them (:136-145): the first point meets every
        # offset, row by row, so offset (a, b) has index a * resolution + b
        pts = torch.tensor(list(itertools.product(range(resolution), range(resolution))), device='cpu')
        off = (pts[:, None, :] - pts[None, :, :]).abs()
        self.attention_biases = nn.Parameter(torch.zeros(num_heads, resolution * resolution))
        self.register_buffer('attention_bias_idxs', (off[..., 0] * resolution + off[..., 1]).long())

    @torch.no_grad()
    def train(self, mode=True):
        # the reference's quirk (:151-157): the gathered bias is cached when training mode is left (and on train(True) without a
        # cache); a later change of the parameter in eval mode is not seen
        super().train(mode)
        if mode and hasattr(self, 'ab'):
            del self.ab
        else:
            self.ab = self.attention_biases[:, self.attention_bias_idxs]
        return self

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        if hasattr(self, 'ab'):                      # a plain attribute: it follows the parameters to their device
            self.ab = fn(self.ab)
        return self

    def forward(self, x):
        B, C, H, W = x.shape
        bias = self.attention_biases[:, self.attention_bias_idxs] if self.training else self.ab
        chunks = x.chunk(len(self.qkvs), dim=1)
        outs = []
        feat = chunks[0]
        for i, qkv in enumerate(self.qkvs):
            if i > 0:
                feat = feat + chunks[i]
            feat = qkv(feat)
            q, k, v = feat.view(B, -1, H, W).split([self.key_dim, self.key_dim, self.d], dim=1)
            q = self.dws[i](q)
            q, k, v = q.flatten(2), k.flatten(2), v.flatten(2)
            attn = (q.transpose(-2, -1) @ k) * self.scale + bias[i]
            attn = attn.softmax(dim=-1)
            feat = (v @ attn.transpose(-2, -1)).view(B, self.d, H, W)
            outs.append(feat)
        return self.proj(torch.cat(outs, 1))


def _bf16_autocast(x):
    return x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16


class LocalWindowAttention(nn.Module):
    """:184-247.  `fused_attention`: route eval-mode calls to cream_amd.cga_attn where it is covered."""

    def __init__(self, dim, key_dim, num_heads=8, attn_ratio=4, resolution=14, window_resolution=7, kernels=[5, 5, 5, 5],
                 fused_attention=True):
        super().__init__()
        self.dim = dim
        self.num_heads = num_heads
        self.resolution = resolution
        assert window_resolution > 0, 'window_size must be greater than 0'
        self.window_resolution = window_resolution
        self.fused_attention = fused_attention
        self.attn = CascadedGroupAttention(dim, key_dim, num_heads, attn_ratio=attn_ratio,
                                           resolution=min(window_resolution, resolution), kernels=kernels)

    def is_fused(self, x):
        """The path decision for this input: from the module's state and the tensor's descriptors alone."""
        a = self.attn
        if not self.fused_attention or self.training or not hasattr(a, 'ab') or os.environ.get("CREAM_IRPE_FUSED", "1") == "0":
            return False
        if not _bf16_autocast(x):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in a.parameters())):
            return False
        w = min(self.window_resolution, self.resolution)
        return cga_attn.usable_cga(torch.bfloat16, x.device, self.dim, a.num_heads, a.key_dim, a.d, w, a.kernels,
                                   x.shape[2], x.shape[3])

    def forward_fused(self, x):
        """x (B, C, H, W) -> (B, C, H, W): one launch up to the ReLU, then `proj`'s convolution."""
        a = self.attn
        t = x.permute(0, 2, 3, 1)                   # (B, H, W, C): a view; free of copies for a channels-last x
        if t.dtype != torch.bfloat16 or t.stride(3) != 1 or any(s % 8 for s in t.stride()[:3]) or t.data_ptr() % 16:
            t = t.to(torch.bfloat16).contiguous()
        out = cga_attn.fwd_core(t, cga_attn.fold(a), min(self.window_resolution, self.resolution), a.scale)
        return a.proj[1](out.permute(0, 3, 1, 2))

    def forward(self, x):
        H = W = self.resolution
        B, C, H_, W_ = x.shape
        assert H == H_ and W == W_, 'input feature has wrong size, expect {}, got {}'.format((H, W), (H_, W_))
        if self.is_fused(x):
            return self.forward_fused(x)
        w = self.window_resolution
        if H <= w and W <= w:
            return self.attn(x)
        x = x.permute(0, 2, 3, 1)
        pad_b = (w - H % w) % w
        pad_r = (w - W % w) % w
        padding = pad_b > 0 or pad_r > 0
        if padding:
            x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
        pH, pW = H + pad_b, W + pad_r
        nH, nW = pH // w, pW // w
        x = x.view(B, nH, w, nW, w, C).transpose(2, 3).reshape(B * nH * nW, w, w, C).permute(0, 3, 1, 2)
        x = self.attn(x)
        x = x.permute(0, 2, 3, 1).view(B, nH, nW, w, w, C).transpose(2, 3).reshape(B, pH, pW, C)
        if padding:
            x = x[:, :H, :W].contiguous()
        return x.permute(0, 3, 1, 2)


def _kernel_view(t):
    """(B, H, W, C) -> the same values as a tensor the token kernels take: itself where its dtype, strides and base allow."""
    return t if evit_ffn.view_ok(t) else t.to(torch.bfloat16).contiguous()


def _conv_of(m):
    return m if isinstance(m, nn.Conv2d) else m.c


def dw_ffn_tokens(dw, ffn, t):
    """The pair of `Residual`s dw (depthwise 3 x 3) and ffn on t (B, H, W, C): one launch where `evit_ffn.usable_dwffn` holds,
    the two modules on the NCHW view otherwise."""
    c1 = _conv_of(ffn.m.pw1)
    if evit_ffn.usable_dwffn(torch.bfloat16, t.device, c1.in_channels, c1.out_channels, t.shape[1], t.shape[2]):
        return evit_ffn.fwd_dwffn(_kernel_view(t), evit_ffn.fold_dwffn(dw, ffn))
    return ffn(dw(t.permute(0, 3, 1, 2))).permute(0, 2, 3, 1)


def _is_dw_ffn(m):
    return isinstance(m, nn.Sequential) and len(m) == 2 and all(isinstance(r, Residual) for r in m) and isinstance(m[1].m, FFN)


class EfficientViTBlock(nn.Module):
    """:250-282."""

    def __init__(self, type, ed, kd, nh=8, ar=4, resolution=14, window_resolution=7, kernels=[5, 5, 5, 5], fused_attention=True):
        super().__init__()
        self.dw0 = Residual(Conv2d_BN(ed, ed, 3, 1, 1, groups=ed, bn_weight_init=0., resolution=resolution))
        self.ffn0 = Residual(FFN(ed, int(ed * 2), resolution))
        if type == 's':
            self.mixer = Residual(LocalWindowAttention(ed, kd, nh, attn_ratio=ar, resolution=resolution,
                                                       window_resolution=window_resolution, kernels=kernels,
                                                       fused_attention=fused_attention))
        self.dw1 = Residual(Conv2d_BN(ed, ed, 3, 1, 1, groups=ed, bn_weight_init=0., resolution=resolution))
        self.ffn1 = Residual(FFN(ed, int(ed * 2), resolution))

    def forward(self, x):
        return self.ffn1(self.dw1(self.mixer(self.ffn0(self.dw0(x)))))

    def forward_tokens(self, t):
        """t (B, H, W, C) bf16 -> (B, H, W, C) bf16: four launches where everything is covered (eval mode, no gradients)."""
        t = dw_ffn_tokens(self.dw0, self.ffn0, t)
        m = self.mixer.m
        v = t.permute(0, 3, 1, 2)                   # the NCHW view of the token tensor
        if m.is_fused(v):
            a = m.attn
            o = cga_attn.fwd_core(_kernel_view(t), cga_attn.fold(a), min(m.window_resolution, m.resolution), a.scale)
            proj = _conv_of(a.proj[1])
            if evit_ffn.usable_pw(torch.bfloat16, t.device, proj.in_channels, proj.out_channels):
                t = evit_ffn.fwd_pw_residual(o, _kernel_view(t), evit_ffn.fold_pw(a.proj[1]))
            else:
                t = t + a.proj[1](o.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        else:
            t = t + m(v).permute(0, 2, 3, 1)
        return dw_ffn_tokens(self.dw1, self.ffn1, t)


def _dw_ffn(ed, resolution):
    return nn.Sequential(Residual(Conv2d_BN(ed, ed, 3, 1, 1, groups=ed, resolution=resolution)),
                         Residual(FFN(ed, int(ed * 2), resolution)))


class EfficientViT(nn.Module):
    """:285-356."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, stages=['s', 's', 's'], embed_dim=[64, 128, 192],
                 key_dim=[16, 16, 16], depth=[1, 2, 3], num_heads=[4, 4, 4], window_size=[7, 7, 7], kernels=[5, 5, 5, 5],
                 down_ops=[['subsample', 2], ['subsample', 2], ['']], distillation=False, fused_attention=True, fused_blocks=True):
        super().__init__()
        self.fused_blocks = bool(fused_blocks)
        resolution = img_size
        e0 = embed_dim[0]
        self.patch_embed = nn.Sequential(
            Conv2d_BN(in_chans, e0 // 8, 3, 2, 1, resolution=resolution), nn.ReLU(),
            Conv2d_BN(e0 // 8, e0 // 4, 3, 2, 1, resolution=resolution // 2), nn.ReLU(),
            Conv2d_BN(e0 // 4, e0 // 2, 3, 2, 1, resolution=resolution // 4), nn.ReLU(),
            Conv2d_BN(e0 // 2, e0, 3, 2, 1, resolution=resolution // 8))
        resolution = img_size // patch_size
        attn_ratio = [embed_dim[i] / (key_dim[i] * num_heads[i]) for i in range(len(embed_dim))]
        stages_ = [[], [], [], []]                   # blocks1, blocks2, blocks3 and the overflow slot of a last 'subsample'
        for i, (stg, ed, kd, dpth, nh, ar, wd, do) in enumerate(zip(stages, embed_dim, key_dim, depth, num_heads, attn_ratio,
                                                                    window_size, down_ops)):
            for _ in range(dpth):
                stages_[i].append(EfficientViTBlock(stg, ed, kd, nh, ar, resolution, wd, kernels, fused_attention=fused_attention))
            if do[0] == 'subsample':
                # the downsample block opens the NEXT stage: Sequential, PatchMerging, Sequential, then that stage's blocks
                nxt = stages_[i + 1]
                nxt.append(_dw_ffn(embed_dim[i], resolution))
                nxt.append(PatchMerging(*embed_dim[i:i + 2], resolution))
                resolution = (resolution - 1) // do[1] + 1
                nxt.append(_dw_ffn(embed_dim[i + 1], resolution))
        self.blocks1 = nn.Sequential(*stages_[0])
        self.blocks2 = nn.Sequential(*stages_[1])
        self.blocks3 = nn.Sequential(*stages_[2])
        self.head = BN_Linear(embed_dim[-1], num_classes) if num_classes > 0 else nn.Identity()
        self.distillation = distillation
        if distillation:
            self.head_dist = BN_Linear(embed_dim[-1], num_classes) if num_classes > 0 else nn.Identity()

    def _mixers(self):
        return [m for m in self.modules() if isinstance(m, LocalWindowAttention)]

    @property
    def fused_attention(self):
        return all(m.fused_attention for m in self._mixers())

    @fused_attention.setter
    def fused_attention(self, flag):
        for m in self._mixers():
            m.fused_attention = bool(flag)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {k for k in self.state_dict().keys() if 'attention_biases' in k}

    def is_tokens(self, x):
        """The path decision for this input: from the model's state and the tensor's descriptors alone (the rule of
        `LocalWindowAttention.is_fused`)."""
        if not self.fused_blocks or self.training or os.environ.get("CREAM_IRPE_FUSED", "1") == "0" or not _bf16_autocast(x):
            return False
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())))

    def forward_tokens(self, x):
        """x (B, 3, H, W) -> the pooled features (B, C): the map stays (B, H, W, C) bf16 from the stem to the pooling."""
        t = _kernel_view(self.patch_embed(x).permute(0, 2, 3, 1))
        for stage in (self.blocks1, self.blocks2, self.blocks3):
            for m in stage:
                if isinstance(m, EfficientViTBlock) and hasattr(m, 'mixer'):
                    t = m.forward_tokens(t)
                elif _is_dw_ffn(m):
                    t = dw_ffn_tokens(m[0], m[1], t)
                else:                               # PatchMerging: the framework, on the channels-last view
                    t = m(t.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        return t.mean((1, 2))

    def forward(self, x):
        if self.is_tokens(x):
            x = self.forward_tokens(x)
        else:
            x = self.blocks3(self.blocks2(self.blocks1(self.patch_embed(x))))
            x = F.adaptive_avg_pool2d(x, 1).flatten(1)
        if not self.distillation:
            return self.head(x)
        x = self.head(x), self.head_dist(x)
        return x if self.training else (x[0] + x[1]) / 2


# ---- the published configurations (build.py:10-68) and factories (:71-171) ------------------------------------------------------
CONFIGS = {
    'EfficientViT_M0': dict(img_size=224, patch_size=16, embed_dim=[64, 128, 192], depth=[1, 2, 3], num_heads=[4, 4, 4],
                            window_size=[7, 7, 7], kernels=[5, 5, 5, 5]),
    'EfficientViT_M1': dict(img_size=224, patch_size=16, embed_dim=[128, 144, 192], depth=[1, 2, 3], num_heads=[2, 3, 3],
                            window_size=[7, 7, 7], kernels=[7, 5, 3, 3]),
    'EfficientViT_M2': dict(img_size=224, patch_size=16, embed_dim=[128, 192, 224], depth=[1, 2, 3], num_heads=[4, 3, 2],
                            window_size=[7, 7, 7], kernels=[7, 5, 3, 3]),
    'EfficientViT_M3': dict(img_size=224, patch_size=16, embed_dim=[128, 240, 320], depth=[1, 2, 3], num_heads=[4, 3, 4],
                            window_size=[7, 7, 7], kernels=[5, 5, 5, 5]),
    'EfficientViT_M4': dict(img_size=224, patch_size=16, embed_dim=[128, 256, 384], depth=[1, 2, 3], num_heads=[4, 4, 4],
                            window_size=[7, 7, 7], kernels=[7, 5, 3, 3]),
    'EfficientViT_M5': dict(img_size=224, patch_size=16, embed_dim=[192, 288, 384], depth=[1, 3, 4], num_heads=[3, 3, 4],
                            window_size=[7, 7, 7], kernels=[7, 5, 3, 3]),
}


def replace_batchnorm(net):
    """:173-180: every module with a `fuse()` becomes its fused form, every remaining BatchNorm2d an Identity."""
    for name, child in net.named_children():
        if hasattr(child, 'fuse'):
            setattr(net, name, child.fuse())
        elif isinstance(child, nn.BatchNorm2d):
            setattr(net, name, nn.Identity())
        else:
            replace_batchnorm(child)


def load_checkpoint_state_dict(model, state):
    """The factories' loading rule (:78-83): a checkpoint entry whose shape differs from the model's (a 2-d weight of what is a
    1 x 1 convolution here) gets two trailing axes, then a strict `load_state_dict`."""
    own = model.state_dict()
    state = {k: (v[:, :, None, None] if k in own and own[k].shape != v.shape else v) for k, v in state.items()}
    return model.load_state_dict(state)


def _factory(name):
    def make(num_classes=1000, pretrained=False, distillation=False, fuse=False, pretrained_cfg=None, model_cfg=None, **kwargs):
        if pretrained:
            raise RuntimeError(f"{name}: nothing is downloaded here; build the model and use load_checkpoint_state_dict")
        model = EfficientViT(num_classes=num_classes, distillation=distillation, **(model_cfg or CONFIGS[name]), **kwargs)
        if fuse:
            replace_batchnorm(model)
        return model
    make.__name__ = make.__qualname__ = name
    return make


EfficientViT_M0 = _factory('EfficientViT_M0')
EfficientViT_M1 = _factory('EfficientViT_M1')
EfficientViT_M2 = _factory('EfficientViT_M2')
EfficientViT_M3 = _factory('EfficientViT_M3')
EfficientViT_M4 = _factory('EfficientViT_M4')
EfficientViT_M5 = _factory('EfficientViT_M5')
