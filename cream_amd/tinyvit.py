"""TinyViT — host-side mirror of TinyViT/models/tiny_vit.py (`Conv2d_BN` :28-50, `PatchEmbed` :64-81, `MBConv` :84-122,
`PatchMerging` :125-151, `ConvLayer` :154-190, `Mlp` :193-213, `Attention` :216-286, `TinyViTBlock` :289-383, `BasicLayer`
:386-450, `TinyViT` :453-591, the factories :640-704) on the fused window attentions of cream_amd.window_attn (windows up to
8 x 8), cream_amd.window_attn_large (9 x 9 .. 14 x 14) and cream_amd.window_attn_xl (15 x 15 .. 32 x 32: the 384 and 512
models), and on the token-layout depthwise convolution of cream_amd.token_conv.

Same constructor arguments, parameter and buffer names as the reference (`layers.{i}.blocks.{j}.attn.attention_biases`,
`...local_conv.c.weight`, `...local_conv.bn.running_mean`, ...; `attention_bias_idxs` is non-persistent), so the published
state dicts load.  Nothing here downloads: the factories have no `pretrained`.

TinyViT's attention needs no kernel of its own:
  * its bias `attention_biases` (H, w^2), indexed by the offset (|dy|, |dx|), expands exactly into Swin's ((2w-1)^2, H) table
    indexed by (dy, dx) — `expand_offset_bias`; the gradient folds back as a fixed-order sum of at most 4 entries per offset;
  * its projection is packed per head, (B, N, H, [q|k|v], 32); the kernels take three pointers and strides, so the permuted
    VIEW goes in as it is;
  * it has no shift and no mask: geometry (H, W, w, 0, 0).

Two paths through `TinyViTBlock.forward`, chosen separately for its two halves:
  * attention, fused — a device tensor under bf16 autocast, `CREAM_IRPE_FUSED` not 0, the map a multiple of the window (the
    reference would not pad), 32-wide heads and `usable_window` / `usable_large_window` / `usable_xl_window` for the expanded
    table (`TinyViTBlock.attention_route`): norm -> qkv on the whole (B, L, C) map -> the strided view -> `window_attention`
    (w <= 8), `large_window_attention` (9 <= w <= 14) or `xl_window_attention` (15 <= w <= 32, the shapes measured faster:
    `window_attn_xl.routed`) -> proj; no pad, no partition, no (N, N) map.  Everything else (fp32, CPU, padded maps, 64-wide
    heads) is the reference's arithmetic step by step;
  * local convolution, fused — on a device, with or without autocast, when `fused_local_conv` is set and
    `token_conv.usable_token_conv` holds: in training mode the convolution on the token layout, then the block's own
    BatchNorm on (B L, C) samples (same statistics and running updates as the reference's (B, C, H, W)); in eval mode
    BatchNorm folded into taps and bias (`Conv2d_BN.fuse`'s formulas, fp32) and one launch.  `fused_local_conv=False` keeps the
    reference's transposes around `Conv2d` and `BatchNorm2d`.  `CREAM_IRPE_FUSED=0` means the attention only.
The NCHW convolutions of `PatchEmbed`, `MBConv` and `PatchMerging`, LayerNorm, the MLP and the linears stay with the framework.
"""
import itertools
from functools import lru_cache

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

from . import token_conv, window_attn, window_attn_large, window_attn_xl
from .rpe_attention import DropPath

HEAD_DIM = 32


def _pair(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


def _trunc_normal(t, std=.02):
    return nn.init.trunc_normal_(t, std=std, a=-2., b=2.)


# ---- the offset bias as a Swin table ----------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def offset_bias_index(w):
    """-> (src ((2w-1)^2), fold (w^2, 4), valid (w^2, 4)) for a w x w window.  Swin entry e = (dy + w - 1)(2w - 1) + (dx + w - 1)
    reads offset src[e] = |dy| w + |dx|; offset (a, b) is read by the entries fold[a w + b, k] with valid[.., k]: (a, b), (a, -b),
    (-a, b), (-a, -b), the duplicates at a == 0 or b == 0 marked invalid."""
    d = torch.arange(-(w - 1), w, device='cpu')      # host tensors, also under a device context
    src = (d.abs().view(-1, 1) * w + d.abs().view(1, -1)).reshape(-1)
    a = torch.arange(w, device='cpu').view(-1, 1).expand(w, w).reshape(-1)
    b = torch.arange(w, device='cpu').view(1, -1).expand(w, w).reshape(-1)
    entry = lambda dy, dx: (dy + w - 1) * (2 * w - 1) + (dx + w - 1)          # noqa: E731
    fold = torch.stack([entry(a, b), entry(a, -b), entry(-a, b), entry(-a, -b)], 1)
    valid = torch.stack([torch.ones_like(a, dtype=torch.bool), b > 0, a > 0, (a > 0) & (b > 0)], 1)
    return src, torch.where(valid, fold, torch.zeros_like(fold)), valid


class _ExpandOffsetBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ab, src, fold, valid):
        ctx.save_for_backward(fold, valid)
        return ab.float()[:, src].t().contiguous()

    @staticmethod
    def backward(ctx, g):
        fold, valid = ctx.saved_tensors
        t = torch.where(valid.unsqueeze(-1), g[fold], torch.zeros((), dtype=g.dtype, device=g.device))       # (w^2, 4, H)
        d = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]                                                         # fixed order
        return d.t().contiguous(), None, None, None


def expand_offset_bias(attention_biases, w, index=None):
    """attention_biases (H, w^2) -> the ((2w-1)^2, H) fp32 contiguous relative-position table that, gathered through Swin's
    `relative_position_index`, equals `attention_biases[:, attention_bias_idxs]` bit for bit.  `index`: the tensors of
    `offset_bias_index(w)` on the parameter's device (a module keeps its own), built here otherwise."""
    if index is None:
        index = tuple(t.to(attention_biases.device) for t in offset_bias_index(w))
    return _ExpandOffsetBias.apply(attention_biases, *index)


# ---- the modules --------------------------------------------------------------------------------------------------------------
class Conv2d_BN(nn.Sequential):
    """:28-50."""

    def __init__(self, a, b, ks=1, stride=1, pad=0, dilation=1, groups=1, bn_weight_init=1):
        super().__init__()
        self.add_module('c', nn.Conv2d(a, b, ks, stride, pad, dilation, groups, bias=False))
        bn = nn.BatchNorm2d(b)
        nn.init.constant_(bn.weight, bn_weight_init)
        nn.init.constant_(bn.bias, 0)
        self.add_module('bn', bn)

    @staticmethod
    def folded(c, bn):
        """BatchNorm's eval-mode affine map folded into the convolution: -> (weight, bias), the formulas of `fuse`."""
        s = bn.weight / (bn.running_var + bn.eps) ** 0.5
        return c.weight * s[:, None, None, None], bn.bias - bn.running_mean * bn.weight / (bn.running_var + bn.eps) ** 0.5

    @torch.no_grad()
    def fuse(self):
        c, bn = self._modules.values()
        w, b = self.folded(c, bn)
        m = nn.Conv2d(w.size(1) * c.groups, w.size(0), w.shape[2:], stride=c.stride, padding=c.padding, dilation=c.dilation,
                      groups=c.groups)
        m.weight.data.copy_(w)
        m.bias.data.copy_(b)
        return m


class PatchEmbed(nn.Module):
    """:64-81."""

    def __init__(self, in_chans, embed_dim, resolution, activation):
        super().__init__()
        img_size = _pair(resolution)
        self.patches_resolution = (img_size[0] // 4, img_size[1] // 4)
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        n = embed_dim
        self.seq = nn.Sequential(Conv2d_BN(in_chans, n // 2, 3, 2, 1), activation(), Conv2d_BN(n // 2, n, 3, 2, 1))

    def forward(self, x):
        return self.seq(x)


class MBConv(nn.Module):
    """:84-122."""

    def __init__(self, in_chans, out_chans, expand_ratio, activation, drop_path):
        super().__init__()
        self.in_chans = in_chans
        self.hidden_chans = int(in_chans * expand_ratio)
        self.out_chans = out_chans
        self.conv1 = Conv2d_BN(in_chans, self.hidden_chans, ks=1)
        self.act1 = activation()
        self.conv2 = Conv2d_BN(self.hidden_chans, self.hidden_chans, ks=3, stride=1, pad=1, groups=self.hidden_chans)
        self.act2 = activation()
        self.conv3 = Conv2d_BN(self.hidden_chans, out_chans, ks=1, bn_weight_init=0.0)
        self.act3 = activation()
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def forward(self, x):
        shortcut = x
        x = self.act1(self.conv1(x))
        x = self.act2(self.conv2(x))
        x = self.drop_path(self.conv3(x))
        x += shortcut
        return self.act3(x)


class PatchMerging(nn.Module):
    """:125-151."""

    def __init__(self, input_resolution, dim, out_dim, activation):
        super().__init__()
        self.input_resolution = input_resolution
        self.dim = dim
        self.out_dim = out_dim
        self.act = activation()
        self.conv1 = Conv2d_BN(dim, out_dim, 1, 1, 0)
        self.conv2 = Conv2d_BN(out_dim, out_dim, 3, 2, 1, groups=out_dim)
        self.conv3 = Conv2d_BN(out_dim, out_dim, 1, 1, 0)

    def forward(self, x):
        if x.ndim == 3:
            H, W = self.input_resolution
            x = x.view(len(x), H, W, -1).permute(0, 3, 1, 2)
        x = self.act(self.conv1(x))
        x = self.act(self.conv2(x))
        x = self.conv3(x)
        return x.flatten(2).transpose(1, 2)


class ConvLayer(nn.Module):
    """:154-190."""

    def __init__(self, dim, input_resolution, depth, activation, drop_path=0., downsample=None, use_checkpoint=False, out_dim=None,
                 conv_expand_ratio=4.):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            MBConv(dim, dim, conv_expand_ratio, activation, drop_path[i] if isinstance(drop_path, list) else drop_path)
            for i in range(depth)])
        self.downsample = (downsample(input_resolution, dim=dim, out_dim=out_dim, activation=activation)
                           if downsample is not None else None)

    def forward(self, x):
        for blk in self.blocks:
            x = checkpoint.checkpoint(blk, x, use_reentrant=False) if self.use_checkpoint else blk(x)
        return self.downsample(x) if self.downsample is not None else x


class Mlp(nn.Module):
    """:193-213: its own LayerNorm in front."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.norm = nn.LayerNorm(in_features)
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.act = act_layer()
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        x = self.drop(self.act(self.fc1(self.norm(x))))
        return self.drop(self.fc2(x))


class Attention(nn.Module):
    """:216-286.  `forward` is the composed path on partitioned windows; `forward_map` the fused one on the whole map."""

    def __init__(self, dim, key_dim, num_heads=8, attn_ratio=4, resolution=(14, 14)):
        super().__init__()
        assert isinstance(resolution, tuple) and len(resolution) == 2
        self.num_heads = num_heads
        self.scale = key_dim ** -0.5
        self.key_dim = key_dim
        self.nh_kd = nh_kd = key_dim * num_heads
        self.d = int(attn_ratio * key_dim)
        self.dh = int(attn_ratio * key_dim) * num_heads
        self.attn_ratio = attn_ratio
        self.resolution = resolution
        self.norm = nn.LayerNorm(dim)
        self.qkv = nn.Linear(dim, self.dh + nh_kd * 2)
        self.proj = nn.Linear(self.dh, dim)
        self.softmax = nn.Softmax(dim=-1)             # a module without state, so that a test can see the composed branch run
        # the reference numbers the offsets (|dy|, |dx|) in the order it meets them (:237-247): the first point meets every
        # offset, row by row, so offset (a, b) has index a * resolution[1] + b
        r0, r1 = resolution
        pts = torch.tensor(list(itertools.product(range(r0), range(r1))))
        off = (pts[:, None, :] - pts[None, :, :]).abs()
        self.attention_biases = nn.Parameter(torch.zeros(num_heads, r0 * r1))
        self.register_buffer('attention_bias_idxs', (off[..., 0] * r1 + off[..., 1]).long(), persistent=False)
        # the index tensors of `expand_offset_bias`, for the windows the fused kernels cover
        self.fusable = r0 == r1 and r0 <= window_attn_xl.MAX_WINDOW and key_dim == HEAD_DIM and self.d == HEAD_DIM
        if self.fusable:
            for name, t in zip(("_expand_src", "_fold_idx", "_fold_valid"), offset_bias_index(r0)):
                self.register_buffer(name, t.clone(), persistent=False)

    def _index(self):
        return self._expand_src, self._fold_idx, self._fold_valid

    @torch.no_grad()
    def train(self, mode=True):
        # the reference's quirk (:254-260): the gathered bias is cached when training mode is left (and on train(True)
        # without a cache); a later change of the parameter in eval mode is not seen.  The expanded table of the fused path is
        # cached at the same moment.
        super().train(mode)
        if mode and hasattr(self, 'ab'):
            del self.ab
            self.ab_table = None
        else:
            self.ab = self.attention_biases[:, self.attention_bias_idxs]
            self.ab_table = expand_offset_bias(self.attention_biases, self.resolution[0], self._index()) if self.fusable else None

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        if hasattr(self, 'ab'):                      # plain attributes: they follow the parameters to their device
            self.ab = fn(self.ab)
            self.ab_table = fn(self.ab_table) if self.ab_table is not None else None
        return self

    def table(self):
        """The expanded ((2w-1)^2, H) table of this call: from the parameter in training mode, the cached one otherwise."""
        if self.training:
            return expand_offset_bias(self.attention_biases, self.resolution[0], self._index())
        return self.ab_table

    def fused_kind(self, dtype, device, table):
        """None (composed), 'small' (window_attn) or 'large' (window_attn_large) for qkv of this dtype on this device."""
        if not self.fusable or table is None:
            return None
        args = (dtype, device, HEAD_DIM, self.num_heads, self.resolution[0], table)
        if window_attn.usable_window(*args):
            return 'small'
        if window_attn_large.usable_large_window(*args):
            return 'large'
        return None

    def fused_route(self, dtype, device, table):
        """`fused_kind`, and 'xl' (window_attn_xl) for the windows of 15 .. 32 that only the streaming kernels cover."""
        kind = self.fused_kind(dtype, device, table)
        if kind is None and self.fusable and window_attn_xl.usable_xl_window(dtype, device, HEAD_DIM, self.num_heads, self.resolution[0], table):
            return 'xl'
        return kind

    def forward_map(self, x, geometry, kind, table):
        """x (B, Hs*Ws, C) of the whole map -> (B, Hs*Ws, C) after proj, through the fused kernels."""
        B, L, _ = x.shape
        qkv = self.qkv(self.norm(x))                  # per token: commutes with the partition
        packed = qkv.view(B, L, self.num_heads, 3, HEAD_DIM).permute(0, 1, 3, 2, 4)       # (B, L, 3, H, 32), a view
        if kind == 'small':
            out = window_attn.window_attention(packed, self.scale, table, geometry)
        elif kind == 'large':
            out = window_attn_large.large_window_attention(packed, self.scale, table, geometry)
        else:
            out = window_attn_xl.xl_window_attention(packed, self.scale, table, geometry)
        return self.proj(out)

    def forward(self, x):
        B, N, _ = x.shape
        x = self.norm(x)
        qkv = self.qkv(x)
        q, k, v = qkv.view(B, N, self.num_heads, -1).split([self.key_dim, self.key_dim, self.d], dim=3)
        q = q.permute(0, 2, 1, 3)
        k = k.permute(0, 2, 1, 3)
        v = v.permute(0, 2, 1, 3)
        attn = (q @ k.transpose(-2, -1)) * self.scale + (self.attention_biases[:, self.attention_bias_idxs] if self.training else self.ab)
        attn = self.softmax(attn)
        x = (attn @ v).transpose(1, 2).reshape(B, N, self.dh)
        return self.proj(x)


def _bn_tokens(bn, z):
    """`bn` (a BatchNorm2d) on z (N, C) as N samples of C channels: `_BatchNorm.forward` with the 2-d input the module's
    own dimension check refuses — the same statistics, `running_*` update and `num_batches_tracked`."""
    eaf = 0.0 if bn.momentum is None else bn.momentum
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
        eaf = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
    use_batch = bn.training or (bn.running_mean is None and bn.running_var is None)
    keep = not bn.training or bn.track_running_stats
    return F.batch_norm(z, bn.running_mean if keep else None, bn.running_var if keep else None, bn.weight, bn.bias, use_batch, eaf,
                        bn.eps)


class TinyViTBlock(nn.Module):
    """:289-383.  `fused_local_conv`: route the depthwise convolution to cream_amd.token_conv where it is covered."""

    def __init__(self, dim, input_resolution, num_heads, window_size=7, mlp_ratio=4., drop=0., drop_path=0., local_conv_size=3,
                 activation=nn.GELU, fused_local_conv=True):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.num_heads = num_heads
        assert window_size > 0, 'window_size must be greater than 0'
        self.window_size = window_size
        self.mlp_ratio = mlp_ratio
        self.fused_local_conv = fused_local_conv
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        assert dim % num_heads == 0, 'dim must be divisible by num_heads'
        head_dim = dim // num_heads
        self.attn = Attention(dim, head_dim, num_heads, attn_ratio=1, resolution=(window_size, window_size))
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=activation, drop=drop)
        pad = local_conv_size // 2
        self.local_conv = Conv2d_BN(dim, dim, ks=local_conv_size, stride=1, pad=pad, groups=dim)
        self._fold = None

    # ---- the path decisions: from descriptors alone ----
    def attention_kind(self, dtype, device):
        """-> (kind, table) for an input that runs in `dtype` (token_conv.io_dtype) on `device`: 'small' / 'large' and the
        expanded table when the fused attention takes it, else (None, None)."""
        kind, table = self.attention_route(dtype, device)
        return (kind, table) if kind in ('small', 'large') else (None, None)

    def attention_route(self, dtype, device):
        """-> (kind, table) as `attention_kind`, with kind 'xl' for the windows of 15 .. 32 (the 384 and 512 models) that
        cream_amd.window_attn_xl takes; `window_attention` follows this one.  Of those windows only the shapes that were
        measured faster than composed are routed (`window_attn_xl.routed`: in ACCEPTED, not in EXCLUDED); any other keeps the
        composed path it had."""
        H, W = self.input_resolution
        w = self.window_size
        if not self.attn.fusable or torch.device(device).type != 'cuda' or H % w or W % w or dtype != torch.bfloat16:
            return None, None
        table = self.attn.table()
        kind = self.attn.fused_route(dtype, device, table)
        if kind == 'xl' and not window_attn_xl.routed(w, H, W, self.num_heads):
            kind = None
        return kind, (table if kind is not None else None)

    def conv_is_fused(self, dtype, device):
        c = self.local_conv.c
        return bool(self.fused_local_conv and c.bias is None and c.padding_mode == 'zeros' and c.in_channels == c.out_channels == self.dim
                    and token_conv.usable_token_conv(dtype, device, self.dim, c.kernel_size, c.stride, c.padding, c.dilation, c.groups))

    def _folded(self):
        """(taps (C, 1, 3, 3), bias (C)) fp32 of the eval-mode Conv2d_BN.  Cached outside autograd, keyed on the versions (and
        storages) of the five tensors: a `load_state_dict` after `eval()` is seen."""
        c, bn = self.local_conv.c, self.local_conv.bn
        five = (c.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        with torch.autocast(c.weight.device.type, enabled=False):
            if torch.is_grad_enabled() and any(t.requires_grad for t in five):
                w, b = Conv2d_BN.folded(c, bn)
                return w.float().contiguous(), b.float().contiguous()
            key = tuple((t._version, t.data_ptr(), t.dtype) for t in five)
            if self._fold is None or self._fold[0] != key:
                with torch.no_grad():
                    w, b = Conv2d_BN.folded(c, bn)
                self._fold = (key, w.float().contiguous(), b.float().contiguous())
            return self._fold[1:]

    def local_convolution(self, x):
        """x (B, L, C) -> Conv2d_BN of the (H, W) map, on the token layout."""
        H, W = self.input_resolution
        B, L, C = x.shape
        if not self.conv_is_fused(token_conv.io_dtype(x), x.device):
            x = x.transpose(1, 2).reshape(B, C, H, W)
            x = self.local_conv(x)
            return x.view(B, C, L).transpose(1, 2)
        c, bn = self.local_conv.c, self.local_conv.bn
        if bn.training or bn.running_mean is None:
            z = token_conv.token_dwconv3(x, c.weight, None, (H, W))
            # the 2-d view: measured against the module on (B L, C, 1, 1), profiles/NOTES_tinyvit.md
            return _bn_tokens(bn, z.view(B * L, C)).view(B, L, C)
        w, b = self._folded()
        return token_conv.token_dwconv3(x, w, b, (H, W))

    def window_attention(self, x):
        """x (B, L, C) -> the attention of its windows, before the residual."""
        H, W = self.input_resolution
        B, L, C = x.shape
        w = self.window_size
        kind, table = self.attention_route(token_conv.io_dtype(x), x.device)
        if kind is not None:
            return self.attn.forward_map(x, (H, W, w, 0, 0), kind, table)
        if H == w and W == w:
            return self.attn(x)
        x = x.view(B, H, W, C)
        pad_b = (w - H % w) % w
        pad_r = (w - W % w) % w
        padding = pad_b > 0 or pad_r > 0
        if padding:
            x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
        pH, pW = H + pad_b, W + pad_r
        nH, nW = pH // w, pW // w
        x = x.view(B, nH, w, nW, w, C).transpose(2, 3).reshape(B * nH * nW, w * w, C)
        x = self.attn(x)
        x = x.view(B, nH, nW, w, w, C).transpose(2, 3).reshape(B, pH, pW, C)
        if padding:
            x = x[:, :H, :W].contiguous()
        return x.view(B, L, C)

    def forward(self, x):
        H, W = self.input_resolution
        assert x.shape[1] == H * W, "input feature has wrong size"
        x = x + self.drop_path(self.window_attention(x))
        x = self.local_convolution(x)
        return x + self.drop_path(self.mlp(x))

    def extra_repr(self):
        return (f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, "
                f"window_size={self.window_size}, mlp_ratio={self.mlp_ratio}")


class BasicLayer(nn.Module):
    """:386-450."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4., drop=0., drop_path=0., downsample=None,
                 use_checkpoint=False, local_conv_size=3, activation=nn.GELU, out_dim=None, fused_local_conv=True):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            TinyViTBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, window_size=window_size, mlp_ratio=mlp_ratio,
                         drop=drop, drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                         local_conv_size=local_conv_size, activation=activation, fused_local_conv=fused_local_conv)
            for i in range(depth)])
        self.downsample = (downsample(input_resolution, dim=dim, out_dim=out_dim, activation=activation)
                           if downsample is not None else None)

    def forward(self, x):
        for blk in self.blocks:
            x = checkpoint.checkpoint(blk, x, use_reentrant=False) if self.use_checkpoint else blk(x)
        return self.downsample(x) if self.downsample is not None else x

    def extra_repr(self):
        return f"dim={self.dim}, input_resolution={self.input_resolution}, depth={self.depth}"


class TinyViT(nn.Module):
    """:453-591."""

    def __init__(self, img_size=224, in_chans=3, num_classes=1000, embed_dims=[96, 192, 384, 768], depths=[2, 2, 6, 2],
                 num_heads=[3, 6, 12, 24], window_sizes=[7, 7, 14, 7], mlp_ratio=4., drop_rate=0., drop_path_rate=0.1,
                 use_checkpoint=False, mbconv_expand_ratio=4.0, local_conv_size=3, layer_lr_decay=1.0, fused_local_conv=True):
        super().__init__()
        self.num_classes = num_classes
        self.depths = depths
        self.num_layers = len(depths)
        self.mlp_ratio = mlp_ratio
        activation = nn.GELU
        self.patch_embed = PatchEmbed(in_chans=in_chans, embed_dim=embed_dims[0], resolution=img_size, activation=activation)
        res = self.patches_resolution = self.patch_embed.patches_resolution
        dpr = torch.linspace(0, drop_path_rate, sum(depths), device='cpu').tolist()     # host numbers, also under a device context
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            kwargs = dict(dim=embed_dims[i], input_resolution=(res[0] // (2 ** i), res[1] // (2 ** i)), depth=depths[i],
                          drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])],
                          downsample=PatchMerging if i < self.num_layers - 1 else None, use_checkpoint=use_checkpoint,
                          out_dim=embed_dims[min(i + 1, len(embed_dims) - 1)], activation=activation)
            if i == 0:
                layer = ConvLayer(conv_expand_ratio=mbconv_expand_ratio, **kwargs)
            else:
                layer = BasicLayer(num_heads=num_heads[i], window_size=window_sizes[i], mlp_ratio=self.mlp_ratio, drop=drop_rate,
                                   local_conv_size=local_conv_size, fused_local_conv=fused_local_conv, **kwargs)
            self.layers.append(layer)
        self.norm_head = nn.LayerNorm(embed_dims[-1])
        self.head = nn.Linear(embed_dims[-1], num_classes) if num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)
        self.set_layer_lr_decay(layer_lr_decay)

    @property
    def fused_local_conv(self):
        return all(b.fused_local_conv for layer in self.layers[1:] for b in layer.blocks)

    @fused_local_conv.setter
    def fused_local_conv(self, flag):
        for layer in self.layers[1:]:
            for b in layer.blocks:
                b.fused_local_conv = bool(flag)

    def set_layer_lr_decay(self, layer_lr_decay):
        """:526-557: every parameter gets `lr_scale` (decaying from the head towards the stem, per block) and `param_name`."""
        depth = sum(self.depths)
        lr_scales = [layer_lr_decay ** (depth - i - 1) for i in range(depth)]

        def set_scale(m, scale):
            for p in m.parameters():
                p.lr_scale = scale

        set_scale(self.patch_embed, lr_scales[0])
        i = 0
        for layer in self.layers:
            for block in layer.blocks:
                set_scale(block, lr_scales[i])
                i += 1
            if layer.downsample is not None:
                set_scale(layer.downsample, lr_scales[i - 1])
        assert i == depth
        for m in (self.norm_head, self.head):
            set_scale(m, lr_scales[-1])
        for k, p in self.named_parameters():
            p.param_name = k
            assert hasattr(p, 'lr_scale'), k

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            _trunc_normal(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {'attention_biases'}

    def forward_features(self, x):
        x = self.patch_embed(x)
        for layer in self.layers:
            x = layer(x)
        return x.mean(1)

    def forward(self, x):
        return self.head(self.norm_head(self.forward_features(x)))


# ---- the published configurations (:640-704) ----------------------------------------------------------------------------------
def _factory(defaults, kwargs):
    kw = dict(defaults)
    kw.update(kwargs)
    return TinyViT(**kw)


def tiny_vit_5m_224(**kwargs):
    return _factory(dict(embed_dims=[64, 128, 160, 320], depths=[2, 2, 6, 2], num_heads=[2, 4, 5, 10], window_sizes=[7, 7, 14, 7],
                         drop_path_rate=0.0), kwargs)


def tiny_vit_11m_224(**kwargs):
    return _factory(dict(embed_dims=[64, 128, 256, 448], depths=[2, 2, 6, 2], num_heads=[2, 4, 8, 14], window_sizes=[7, 7, 14, 7],
                         drop_path_rate=0.1), kwargs)


def tiny_vit_21m_224(**kwargs):
    return _factory(dict(embed_dims=[96, 192, 384, 576], depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 18], window_sizes=[7, 7, 14, 7],
                         drop_path_rate=0.2), kwargs)


def tiny_vit_21m_384(**kwargs):
    return _factory(dict(img_size=384, embed_dims=[96, 192, 384, 576], depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 18],
                         window_sizes=[12, 12, 24, 12], drop_path_rate=0.1), kwargs)


def tiny_vit_21m_512(**kwargs):
    return _factory(dict(img_size=512, embed_dims=[96, 192, 384, 576], depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 18],
                         window_sizes=[16, 16, 32, 16], drop_path_rate=0.1), kwargs)
