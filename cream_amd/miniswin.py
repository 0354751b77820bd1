"""Mini-Swin (weight-shared Swin Transformer with per-repeat LayerNorms, head transforms and local convolutions) —
host-side mirror of MiniViT/Mini-Swin/models/swin_transformer_minivit.py (`WindowAttention` :59-163,
`SwinTransformerBlock` :166-396, `PatchMerging` :399-445, `BasicLayer` :448-534, `PatchEmbed` :537-582,
`SwinTransformerMiniViT` :585-732) on the fused window attention of cream_amd.window_attn.  With the three MiniViT flags
off and `separate_layer_num_list` = depths it is the plain Swin Transformer of the same directory (the distillation teacher).

One `SwinTransformerBlock` (qkv, proj, Mlp, the bias table: the shared weights) runs `share_num` times in a row, the
cyclic shift alternating from `is_init_window_shift`; what is NOT shared is picked by the repeat index: the LayerNorms
(`norm1_list`, `norm2_list`), the two nn.Linear(H, H) over the heads of the attention map (`proj_l` before the softmax,
`proj_w` after it), the LayerNorm + depthwise 7x7 convolution between attention and MLP (`local_norm_list`,
`local_conv_list`) and the drop-path rate.  Same constructor arguments, parameter and buffer names as the reference
(`layers.{i}.blocks.{j}.attn.relative_position_bias_table`, `...attn.relative_position_index`, `...attn_mask`,
`...norm1_list.{r}.weight`, `...proj_l.{r}.weight`), so Mini-Swin checkpoints load.

As in the reference, a block whose map is larger than the window always has `shift_size = window_size // 2` and its
`attn_mask` is passed to the attention in EVERY repeat, rolled or not.

Two paths through `SwinTransformerBlock.forward_feature`:
  * fused — under bf16 autocast on a device where `window_attn.usable_window` agrees: norm1 -> qkv on (B, L, C) ->
    `window_attn.window_attention` -> proj; no roll, no partition, no (N, N) map;
  * fused, window 12 (Mini-Swin-B at 384 and its plain Swin-B teacher) — the measured shapes of
    `window_attn_mix_large.ACCEPTED` (head transforms, 9 <= w <= 12, at most 16 heads) go to
    `window_attn_mix_large.mix_large_window_attention`, those of `PLAIN_ACCEPTED` (no head transforms, 9 <= w <= 14) to
    `window_attn_large.large_window_attention`, the same way;
  * composed — everything else (fp32, CPU, an unmeasured shape at window 9 and above, active attention dropout, more than 16
    mixed heads): the reference's arithmetic step by step.
The local convolution (`SwinTransformerBlock.local_convolution`): LayerNorm, then `x + conv(x)` —
  * fused — on a device, with or without autocast, when `fused_local_conv` is set and `token_conv.usable_token_conv7` holds
    for the repeat's `nn.Conv2d`: the LayerNorm's output goes to `token_conv.token_dwconv7(..., residual=True)` on the token
    layout in its own dtype.  Under bf16 autocast that is fp32 (LayerNorm's output and the residual stream are fp32 there), so
    the branch spends no bf16 rounding — deliberately unlike the framework's autocast convolution, which rounds input, taps
    and output to bf16.  Every shape of the published recipes measured faster fused than composed
    (profiles/NOTES_miniswin_local_conv.md), so no shape is excluded on speed grounds;
  * composed — CPU tensors, `fused_local_conv=False`, a convolution someone replaced, fp16: the reference's transposes to NCHW
    and back around `nn.Conv2d`.
`CREAM_IRPE_FUSED` switches the attention only.  Patch merging and patch embedding stay with the framework.

The distilling models (`SwinTransformerMiniViTDistill`, mirror of swin_transformer_minivit_distill.py:447-621, and the plain
Swin teacher `SwinTransformerDistill`, mirror of swin_transformer_distill.py) return, per layer id listed, a TAP of the
attention's q, k, v — a `minivit_distill.QkvTap` on the fused path, the reference's tuple of windowed views on the composed one
— and the block's output; cream_amd.minivit_distill turns them into the relation losses.
"""
import torch
import torch.nn as nn

from . import token_conv, window_attn, window_attn_large, window_attn_mix_large
from .minivit_distill import QkvTap
from .rpe_attention import DropPath


def _pair(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


def _trunc_normal(t, std=.02):
    return nn.init.trunc_normal_(t, std=std, a=-2., b=2.)


class Mlp(nn.Module):
    """:7-24."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


def window_partition(x, window_size):
    """(B, H, W, C) -> (B * nW, w, w, C), windows row-major (:27-39)."""
    B, H, W, C = x.shape
    x = x.view(B, H // window_size, window_size, W // window_size, window_size, C)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, window_size, window_size, C)


def window_reverse(windows, window_size, H, W):
    """(B * nW, w, w, C) -> (B, H, W, C) (:42-56)."""
    B = windows.shape[0] // ((H // window_size) * (W // window_size))
    x = windows.view(B, H // window_size, W // window_size, window_size, window_size, -1)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)


def relative_position_index(wh, ww):
    """(wh*ww, wh*ww) table row of every (query, key) pair: (iy-jy+wh-1)(2ww-1) + (ix-jx+ww-1) (:94-103)."""
    ys, xs = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")
    ys, xs = ys.flatten(), xs.flatten()
    return (ys[:, None] - ys[None, :] + wh - 1) * (2 * ww - 1) + (xs[:, None] - xs[None, :] + ww - 1)


def shift_mask(H, W, window_size, shift_size):
    """(nW, N, N) of {0, -100}: tokens of one window that come from different regions of the rolled map (:233-252)."""
    img = torch.zeros((1, H, W, 1))
    cuts = (slice(0, -window_size), slice(-window_size, -shift_size), slice(-shift_size, None))
    n = 0
    for hs in cuts:
        for ws in cuts:
            img[:, hs, ws, :] = n
            n += 1
    ids = window_partition(img, window_size).view(-1, window_size * window_size)
    diff = ids.unsqueeze(1) - ids.unsqueeze(2)
    return torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff))


class WindowAttention(nn.Module):
    """:59-163.  `forward` is the composed path on partitioned windows; `forward_map` the fused one on the whole map."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.dim = dim
        self.window_size = _pair(window_size)
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.softmax = nn.Softmax(dim=-1)
        wh, ww = self.window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wh - 1) * (2 * ww - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(wh, ww))
        _trunc_normal(self.relative_position_bias_table)

    def usable(self, qkv, window_size, proj_l, proj_w):
        """Whether the fused kernels take this call (window_size: the block's, which a small map may have clamped)."""
        if self.window_size[0] != self.window_size[1] or window_size != self.window_size[0]:
            return False
        return window_attn.usable_window(qkv.dtype, qkv.device, self.dim // self.num_heads, self.num_heads, window_size,
                                         self.relative_position_bias_table, proj_l, proj_w,
                                         dropout_p=self.attn_drop.p if self.training else 0.0)

    def route(self, qkv, window_size, Hs, Ws, proj_l, proj_w):
        """Which fused kernels take this call, from descriptors alone: 'window' (window_attn, w * w <= 64), 'mix_large'
        (window_attn_mix_large: head transforms at 9 <= w <= 12) or 'large' (window_attn_large: no head transforms at
        9 <= w <= 14), the last two only for the measured shapes of window_attn_mix_large.ACCEPTED / PLAIN_ACCEPTED; None:
        the composed path."""
        if self.usable(qkv, window_size, proj_l, proj_w):
            return "window"
        if self.window_size[0] != self.window_size[1] or window_size != self.window_size[0]:
            return None
        args = (qkv.dtype, qkv.device, self.dim // self.num_heads, self.num_heads, window_size, self.relative_position_bias_table)
        p = self.attn_drop.p if self.training else 0.0
        if proj_l is not None and proj_w is not None:
            if (window_attn_mix_large.routed(window_size, Hs, Ws, self.num_heads)
                    and window_attn_mix_large.usable_mix_large_window(*args, proj_l, proj_w, dropout_p=p)):
                return "mix_large"
        elif proj_l is None and proj_w is None:
            if (window_attn_mix_large.routed_plain(window_size, Hs, Ws, self.num_heads)
                    and window_attn_large.usable_large_window(*args, dropout_p=p)):
                return "large"
        return None

    def forward_map(self, qkv, geometry, proj_l=None, proj_w=None, route="window"):
        """qkv (B, Hs*Ws, 3C) of the unshifted map -> (B, Hs*Ws, C) after proj, through the fused kernels `route` names."""
        B, L, _ = qkv.shape
        qkv = qkv.view(B, L, 3, self.num_heads, self.dim // self.num_heads)
        if route == "mix_large":
            out = window_attn_mix_large.mix_large_window_attention(qkv, self.scale, self.relative_position_bias_table, geometry,
                                                                   proj_l, proj_w)
        elif route == "large":
            out = window_attn_large.large_window_attention(qkv, self.scale, self.relative_position_bias_table, geometry)
        else:
            out = window_attn.window_attention(qkv, self.scale, self.relative_position_bias_table, geometry, proj_l, proj_w)
        return self.proj_drop(self.proj(out))

    def forward(self, x, mask=None, proj_l=None, proj_w=None):
        B_, N, C = x.shape
        return self.attend(self.qkv(x), mask, proj_l, proj_w)

    def attend(self, qkv, mask=None, proj_l=None, proj_w=None):
        """The reference's arithmetic on partitioned windows: qkv (B * nW, N, 3C) -> (B * nW, N, C) after proj."""
        B_, N, C3 = qkv.shape
        C = C3 // 3
        q, k, v = qkv.reshape(B_, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
        attn = (q * self.scale) @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, -1)
        attn = attn + bias.permute(2, 0, 1).unsqueeze(0)
        if proj_l is not None:
            attn = proj_l(attn.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        if mask is not None:
            nW = mask.shape[0]
            attn = (attn.view(B_ // nW, nW, self.num_heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, self.num_heads, N, N)
        attn = self.softmax(attn)
        if proj_w is not None:
            attn = proj_w(attn.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        attn = self.attn_drop(attn)
        x = (attn @ v).transpose(1, 2).reshape(B_, N, C)
        return self.proj_drop(self.proj(x))

    def extra_repr(self):
        return f'dim={self.dim}, window_size={self.window_size}, num_heads={self.num_heads}'


class SwinTransformerBlock(nn.Module):
    """:166-396.  `fused_local_conv`: route the depthwise 7 x 7 convolution to cream_amd.token_conv where it is covered."""

    def __init__(self, dim, input_resolution, num_heads, window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0.,
                 attn_drop=0., shift_size=0., drop_path=(0,), act_layer=nn.GELU, norm_layer=nn.LayerNorm,
                 is_init_window_shift=False, is_sep_layernorm=False, is_transform_FFN=False, is_transform_heads=False,
                 fused_local_conv=True):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.num_heads = num_heads
        self.window_size = window_size
        self.fused_local_conv = fused_local_conv
        self.mlp_ratio = mlp_ratio
        self.share_num = len(drop_path)
        self.is_init_window_shift = is_init_window_shift
        self.is_sep_layernorm = is_sep_layernorm
        self.is_transform_FFN = is_transform_FFN
        self.is_transform_heads = is_transform_heads

        def per_repeat(make):
            return nn.ModuleList([make() for _ in range(self.share_num)])

        if is_sep_layernorm:
            self.norm1_list = per_repeat(lambda: norm_layer(dim))
        else:
            self.norm1 = norm_layer(dim)
        if is_transform_heads:
            self.proj_l = nn.ModuleList()
            self.proj_w = nn.ModuleList()
            for _ in range(self.share_num):                 # creation order of the reference: l, w, l, w, ...
                self.proj_l.append(nn.Linear(num_heads, num_heads))
                self.proj_w.append(nn.Linear(num_heads, num_heads))
        else:
            self.proj_l = self.proj_w = None
        self.attn = WindowAttention(dim, window_size=_pair(window_size), num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                    attn_drop=attn_drop, proj_drop=drop)
        if min(input_resolution) <= self.window_size:        # the map is one window: no partition, no shift (:227-230)
            shift_size = 0
            self.window_size = min(input_resolution)
        assert 0 <= shift_size < self.window_size, "shift_size must in 0-window_size"
        self.shift_size = int(shift_size)
        self.register_buffer("attn_mask", shift_mask(*input_resolution, self.window_size, self.shift_size)
                             if self.shift_size > 0 else None)
        if is_sep_layernorm:
            self.norm2_list = per_repeat(lambda: norm_layer(dim))
        else:
            self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.drop_path = nn.ModuleList([DropPath(p) if p > 0. else nn.Identity() for p in drop_path])
        if is_transform_FFN:
            self.local_norm_list = nn.ModuleList()
            self.local_conv_list = nn.ModuleList()
            for _ in range(self.share_num):
                self.local_norm_list.append(norm_layer(dim))
                self.local_conv_list.append(nn.Conv2d(dim, dim, 7, 1, 3, groups=dim, bias=qkv_bias))
        else:
            self.local_conv_list = None
        self._taps = None                                    # forward_taps: the list the attention's q, k, v go to

    def forward_feature(self, x, is_shift=False, layer_index=0):
        H, W = self.input_resolution
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        shortcut = x
        x = (self.norm1_list[layer_index] if self.is_sep_layernorm else self.norm1)(x)
        proj_l = self.proj_l[layer_index] if self.is_transform_heads else None
        proj_w = self.proj_w[layer_index] if self.is_transform_heads else None
        shift = self.shift_size if is_shift else 0
        w = self.window_size
        qkv = self.attn.qkv(x)                               # per token: commutes with the roll and the partition
        route = self.attn.route(qkv, w, H, W, proj_l, proj_w)
        if route is not None:
            if self._taps is not None:
                self._taps.append(QkvTap(qkv, (H, W, w, shift)))
            x = self.attn.forward_map(qkv, (H, W, w, shift, self.shift_size), proj_l, proj_w, route)
        else:
            qkv = qkv.view(B, H, W, 3 * C)
            if shift > 0:
                qkv = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2))
            windows = window_partition(qkv, w).reshape(-1, w * w, 3 * C)
            if self._taps is not None:                       # the reference's tuple: (B * nW, N, C) views (:71, :100)
                self._taps.append(windows.view(-1, w * w, 3, C).unbind(2))
            x = self.attn.attend(windows, mask=self.attn_mask, proj_l=proj_l, proj_w=proj_w)      # the mask in every repeat (:312)
            x = window_reverse(x.view(-1, w, w, C), w, H, W)
            if shift > 0:
                x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
            x = x.reshape(B, H * W, C)
        x = shortcut + self.drop_path[layer_index](x)
        if self.local_conv_list is not None:
            x = self.local_convolution(x, layer_index)
        norm2 = self.norm2_list[layer_index] if self.is_sep_layernorm else self.norm2
        return x + self.drop_path[layer_index](self.mlp(norm2(x)))

    def local_conv_is_fused(self, dtype, device, layer_index=0):
        """Whether repeat `layer_index`'s convolution goes to the token-layout kernels for an input of this dtype on this
        device, from descriptors alone."""
        c = self.local_conv_list[layer_index]
        return bool(self.fused_local_conv and type(c) is nn.Conv2d and c.padding_mode == 'zeros'
                    and c.in_channels == c.out_channels == self.dim and c.weight.dtype == torch.float32
                    and token_conv.usable_token_conv7(dtype, device, self.dim, c.kernel_size, c.stride, c.padding, c.dilation,
                                                      c.groups))

    def local_convolution(self, x, layer_index):
        """:328-332: x (B, H*W, C) -> y + conv(y) with y = local_norm(x), repeat `layer_index`'s LayerNorm and depthwise 7 x 7
        convolution.  The fused branch hands the LayerNorm's output to the token-layout kernel in its own dtype — fp32 under
        bf16 autocast, so it spends no bf16 rounding where the framework's autocast convolution rounds input, taps and output
        to bf16; the composed branch is the reference's lines."""
        H, W = self.input_resolution
        B, L, C = x.shape
        x = self.local_norm_list[layer_index](x)
        if self.local_conv_is_fused(x.dtype, x.device, layer_index):
            c = self.local_conv_list[layer_index]
            return token_conv.token_dwconv7(x, c.weight, c.bias, (H, W), residual=True)
        x = x.permute(0, 2, 1).reshape(B, C, H, W)
        x = x + self.local_conv_list[layer_index](x)
        return x.reshape(B, C, H * W).permute(0, 2, 1)

    def forward(self, x):
        shift = self.is_init_window_shift
        for index in range(self.share_num):
            x = self.forward_feature(x, shift, index)
            shift = not shift
        return x

    def forward_taps(self, x):
        """`forward` of the distilling block (swin_transformer_minivit_distill.py:291-300): -> (x, one tap of q, k, v per
        repeat, the output of every repeat)."""
        self._taps, hidden = [], []
        try:
            shift = self.is_init_window_shift
            for index in range(self.share_num):
                x = self.forward_feature(x, shift, index)
                hidden.append(x)
                shift = not shift
            return x, self._taps, hidden
        finally:
            self._taps = None

    def extra_repr(self):
        return (f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, "
                f"window_size={self.window_size}, shift_size={self.shift_size}, mlp_ratio={self.mlp_ratio}")

    def custom_init_weights(self):
        """The head transforms start as truncated normals with zero bias (:350-372)."""
        for lst in (self.proj_l, self.proj_w):
            for m in (lst or ()):
                _trunc_normal(m.weight)
                nn.init.constant_(m.bias, 0)


class PatchMerging(nn.Module):
    """:399-445: 2 x 2 neighbours concatenated (order (0,0), (1,0), (0,1), (1,1)), LayerNorm, 4C -> 2C without bias."""

    def __init__(self, input_resolution, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.input_resolution = input_resolution
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x):
        H, W = self.input_resolution
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        assert H % 2 == 0 and W % 2 == 0, f"x size ({H}*{W}) are not even."
        x = x.view(B, H, W, C)
        x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
        return self.reduction(self.norm(x.view(B, -1, 4 * C)))

    def extra_repr(self):
        return f"input_resolution={self.input_resolution}, dim={self.dim}"


class BasicLayer(nn.Module):
    """:448-534: `separate_layer_num` blocks, each shared depth // separate_layer_num times."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0.,
                 attn_drop=0., drop_path=(0.,), norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False,
                 is_sep_layernorm=False, is_transform_FFN=False, is_transform_heads=False, separate_layer_num=1,
                 fused_local_conv=True):
        super().__init__()
        assert isinstance(drop_path, list)
        self.dim = dim
        self.input_resolution = input_resolution
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.share_times = depth // separate_layer_num
        self.separate_layer_num = separate_layer_num
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, window_size=window_size,
                                 shift_size=window_size // 2, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop,
                                 attn_drop=attn_drop,
                                 drop_path=drop_path[i * self.share_times:min((i + 1) * self.share_times, depth)],
                                 norm_layer=norm_layer, is_init_window_shift=(i * self.share_times) % 2 == 1,
                                 is_sep_layernorm=is_sep_layernorm, is_transform_FFN=is_transform_FFN,
                                 is_transform_heads=is_transform_heads, fused_local_conv=fused_local_conv)
            for i in range(separate_layer_num)])
        self.downsample = downsample(input_resolution, dim=dim, norm_layer=norm_layer) if downsample is not None else None

    def forward(self, x):
        for blk in self.blocks:
            if self.use_checkpoint:
                from torch.utils import checkpoint
                x = checkpoint.checkpoint(blk, x)
            else:
                x = blk(x)
        return self.downsample(x) if self.downsample is not None else x

    def forward_taps(self, x):
        """The distilling layer (swin_transformer_minivit_distill.py:422-434): the hidden states are the blocks' outputs before
        patch merging."""
        taps, hidden = [], []
        for blk in self.blocks:
            x, t, h = blk.forward_taps(x)
            taps += t
            hidden += h
        return (self.downsample(x) if self.downsample is not None else x), taps, hidden

    def extra_repr(self):
        return f"dim={self.dim}, input_resolution={self.input_resolution}, depth={self.depth}"


class SwinBasicLayer(BasicLayer):
    """A stage of the plain Swin Transformer (swin_transformer_distill.py:235-300): `depth` unshared blocks, the odd ones
    shifted, the even ones without shift AND without mask.  Takes BasicLayer's arguments; the MiniViT ones are ignored."""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0.,
                 attn_drop=0., drop_path=(0.,), norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False, **minivit):
        nn.Module.__init__(self)
        self.dim = dim
        self.input_resolution = input_resolution
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.share_times = 1
        self.separate_layer_num = depth
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, window_size=window_size,
                                 shift_size=0 if i % 2 == 0 else window_size // 2, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                 qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 drop_path=[drop_path[i] if isinstance(drop_path, (list, tuple)) else drop_path],
                                 norm_layer=norm_layer, is_init_window_shift=i % 2 == 1,
                                 fused_local_conv=minivit.get("fused_local_conv", True))
            for i in range(depth)])
        self.downsample = downsample(input_resolution, dim=dim, norm_layer=norm_layer) if downsample is not None else None


class PatchEmbed(nn.Module):
    """:537-582."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.img_size = _pair(img_size)
        self.patch_size = _pair(patch_size)
        self.patches_resolution = [self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1]]
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        B, C, H, W = x.shape
        assert (H, W) == self.img_size, f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."
        x = self.proj(x).flatten(2).transpose(1, 2)
        return self.norm(x) if self.norm is not None else x


class SwinTransformerMiniViT(nn.Module):
    """:585-732."""
    layer_class = BasicLayer

    def __init__(self, img_size=224, patch_size=4, in_chans=3, num_classes=1000, embed_dim=96, depths=(2, 2, 6, 2),
                 num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True, use_checkpoint=False,
                 is_sep_layernorm=False, is_transform_FFN=False, is_transform_heads=False, separate_layer_num_list=(1, 1, 2, 1),
                 fused_local_conv=True, **kwargs):
        super().__init__()
        self.num_classes = num_classes
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.ape = ape
        self.patch_norm = patch_norm
        self.num_features = int(embed_dim * 2 ** (self.num_layers - 1))
        self.mlp_ratio = mlp_ratio
        self.is_sep_layernorm = is_sep_layernorm
        self.is_transform_FFN = is_transform_FFN
        self.is_transform_heads = is_transform_heads
        self.separate_layer_num_list = separate_layer_num_list
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if patch_norm else None)
        res = self.patches_resolution = self.patch_embed.patches_resolution
        if ape:
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches, embed_dim))
            _trunc_normal(self.absolute_pos_embed)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            self.layers.append(self.layer_class(
                dim=int(embed_dim * 2 ** i), input_resolution=(res[0] // 2 ** i, res[1] // 2 ** i), depth=depths[i],
                num_heads=num_heads[i], window_size=window_size, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                downsample=PatchMerging if i < self.num_layers - 1 else None, use_checkpoint=use_checkpoint,
                is_sep_layernorm=is_sep_layernorm, is_transform_FFN=is_transform_FFN, is_transform_heads=is_transform_heads,
                separate_layer_num=separate_layer_num_list[i], fused_local_conv=fused_local_conv))
        self.norm = norm_layer(self.num_features)
        self.avgpool = nn.AdaptiveAvgPool1d(1)
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)
        for m in self.modules():
            if isinstance(m, SwinTransformerBlock):
                m.custom_init_weights()

    @property
    def fused_local_conv(self):
        """Whether every block routes its local convolution to cream_amd.token_conv where it is covered (a plain attribute of
        the blocks: no parameter, no buffer)."""
        return all(b.fused_local_conv for layer in self.layers for b in layer.blocks)

    @fused_local_conv.setter
    def fused_local_conv(self, flag):
        for layer in self.layers:
            for b in layer.blocks:
                b.fused_local_conv = bool(flag)

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
    def no_weight_decay(self):
        return {'absolute_pos_embed'}

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {'relative_position_bias_table'}

    def forward_features(self, x):
        x = self.patch_embed(x)
        if self.ape:
            x = x + self.absolute_pos_embed
        x = self.pos_drop(x)
        for layer in self.layers:
            x = layer(x)
        x = self.norm(x)
        return torch.flatten(self.avgpool(x.transpose(1, 2)), 1)

    def forward(self, x):
        return self.head(self.forward_features(x))


class SwinTransformerMiniViTDistill(SwinTransformerMiniViT):
    """swin_transformer_minivit_distill.py:447-621: SwinTransformerMiniViT that also returns, for the layer ids listed (counted
    over the repeats of all stages), a tap of the attention's q, k, v and the hidden state; a student carries one
    `fit_dense_C.{i}` = nn.Linear(embed_dim 2^i, fit_size_C 2^i) per stage for the plain hidden loss."""

    def __init__(self, *args, is_student=False, fit_size_C=128, **kwargs):
        super().__init__(*args, **kwargs)
        self.is_student = is_student
        self.fit_size_C = fit_size_C
        self.fit_dense_C = nn.ModuleList()
        if is_student:
            for i in range(self.num_layers):
                self.fit_dense_C.append(nn.Linear(int(self.embed_dim * 2 ** i), int(fit_size_C * 2 ** i)))
        self.fit_dense_C.apply(self._init_weights)

    def forward_features(self, x, layer_id_list=(), is_hidden_org=True):
        """:580-604."""
        x = self.patch_embed(x)
        if self.ape:
            x = x + self.absolute_pos_embed
        x = self.pos_drop(x)
        layer_id = 0
        taps_out, hidden_out = [], []
        for i, layer in enumerate(self.layers):
            x, taps, hidden = layer.forward_taps(x)
            for index in range(len(taps)):
                if index + layer_id in layer_id_list:
                    taps_out.append(taps[index])
                    fit = self.is_student and not is_hidden_org
                    hidden_out.append(self.fit_dense_C[i](hidden[index]) if fit else hidden[index])
            layer_id += len(taps)
        x = self.norm(x)
        return torch.flatten(self.avgpool(x.transpose(1, 2)), 1), taps_out, hidden_out

    def forward(self, x, layer_id_list=(), is_attn_loss=False, is_hidden_loss=False, is_hidden_org=True):
        """:606-621: logits | (logits, taps) | (logits, hidden) | (logits, taps, hidden)."""
        x, taps, hidden = self.forward_features(x, layer_id_list, is_hidden_org=is_hidden_org)
        x = self.head(x)
        if is_attn_loss and is_hidden_loss:
            return x, taps, hidden
        if is_attn_loss:
            return x, taps
        if is_hidden_loss:
            return x, hidden
        return x


class SwinTransformerDistill(SwinTransformerMiniViTDistill):
    """swin_transformer_distill.py:309-464: the plain Swin Transformer (the teacher) with the same taps, under the plain Swin's
    parameter names (`layers.{i}.blocks.{j}.norm1`, `.attn.*`, `.norm2`, `.mlp.*`; `attn_mask` on the shifted blocks only), so
    that a Swin checkpoint loads."""
    layer_class = SwinBasicLayer

    def __init__(self, img_size=224, patch_size=4, in_chans=3, num_classes=1000, embed_dim=96, depths=(2, 2, 6, 2),
                 num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True, use_checkpoint=False,
                 is_student=False, fit_size_C=128, fused_local_conv=True, **kwargs):
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, num_classes=num_classes, embed_dim=embed_dim,
                         depths=depths, num_heads=num_heads, window_size=window_size, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                         qk_scale=qk_scale, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate,
                         norm_layer=norm_layer, ape=ape, patch_norm=patch_norm, use_checkpoint=use_checkpoint,
                         separate_layer_num_list=list(depths), is_student=is_student, fit_size_C=fit_size_C,
                         fused_local_conv=fused_local_conv)

    def forward(self, x, layer_id_list=(), is_attn_loss=False, is_hidden_loss=False, is_hidden_org=False):
        return super().forward(x, layer_id_list, is_attn_loss, is_hidden_loss, is_hidden_org)


# the published Mini-Swin recipes (Mini-Swin/configs/swin_{tiny,small,base}_patch4_window7_224_minivit_sharenum*.yaml)
_SWIN = dict(tiny=dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], separate_layer_num_list=[1, 1, 1, 1],
                       drop_path_rate=0.0),
             small=dict(embed_dim=96, depths=[2, 2, 18, 2], num_heads=[3, 6, 12, 24], separate_layer_num_list=[1, 1, 9, 1],
                        drop_path_rate=0.1),
             base=dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], separate_layer_num_list=[1, 1, 9, 1],
                       drop_path_rate=0.2))


def mini_swin(size='tiny', img_size=224, **kwargs):
    """Mini-Swin-{T,S,B} at 224 with window 7: every stage's blocks shared (tiny) or shared in pairs in stage 3 (small,
    base), per-repeat LayerNorms, head transforms and local convolutions on.  `mini_swin('base', img_size=384,
    window_size=12)` is the 224-to-384 fine-tuning recipe (heads 4 / 8 / 16 / 32 on maps of 96 / 48 / 24 / 12).
    `fused_local_conv=False` keeps the local convolutions on the framework's path."""
    kw = dict(img_size=img_size, patch_size=4, window_size=7, mlp_ratio=4., qkv_bias=True, is_sep_layernorm=True,
              is_transform_FFN=True, is_transform_heads=True)
    kw.update(_SWIN[size])
    kw.update(kwargs)
    return SwinTransformerMiniViT(**kw)
