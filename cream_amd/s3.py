"""S3 (AutoFormerV2: a Swin Transformer with 32-wide heads and per-stage, per-block widths, head counts, window sizes and
MLP ratios) — host-side mirror of AutoFormerV2/model/SSS.py (`WindowAttention` :58-153, `SwinTransformerBlock` :156-281,
`PatchMerging` :284-330, `BasicLayer` :333-400, `PatchEmbed` :403-448, `SSSTransformer` :451-577) on the fused window
attentions of cream_amd.window_attn (windows up to 8x8) and cream_amd.window_attn_large (9x9 .. 14x14).

Same constructor arguments, parameter and buffer names as the reference (`layers.{i}.blocks.{j}.attn.qkv.weight`,
`...attn.relative_position_bias_table`, `...attn.relative_position_index`, `...attn_mask` on the shifted blocks,
`layers.{i}.downsample.reduction.weight`), so the published S3-{T,S,B} state dicts load.  What differs from
cream_amd.miniswin:
  * `embed_dim`, `num_heads`, `window_size`, `mlp_ratio` are lists — per stage, and per block within a stage;
  * the heads are 32 wide whatever the width: `qkv = nn.Linear(dim, num_heads * 32 * 3)` (:78, :98);
  * `PatchMerging` maps 4 dim to the NEXT stage's width `out_dim` (:293-298);
  * the block clamps `window_size` to the map BEFORE it builds its attention (:185-194), so S3-S's last stage (7 x 7 map,
    window 14) owns a 13^2-row table;
  * even blocks have no shift and no mask, odd ones both (:367).

Two paths through `SwinTransformerBlock.forward`, as in miniswin:
  * fused — under bf16 autocast on a device: norm1 -> qkv on (B, L, C) -> `window_attn.window_attention` (w <= 8) or
    `window_attn_large.large_window_attention` (9 <= w <= 14) -> proj; no roll, no partition, no (N, N) map;
  * composed — everything else (fp32, CPU, active attention dropout, CREAM_IRPE_FUSED=0, other windows): the reference's
    arithmetic step by step.
Patch embedding, patch merging, LayerNorm, MLP and the linears stay with the framework.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import window_attn, window_attn_large
from .miniswin import Mlp, PatchEmbed, _pair, _trunc_normal, relative_position_index, shift_mask, window_partition, window_reverse
from .rpe_attention import DropPath

HEAD_DIM = 32


class WindowAttention(nn.Module):
    """:58-153.  `forward` is the composed path on partitioned windows; `forward_map` the fused one on the whole map."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.dim = dim
        self.window_size = _pair(window_size)
        self.num_heads = num_heads
        self.scale = qk_scale or HEAD_DIM ** -0.5
        wh, ww = self.window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wh - 1) * (2 * ww - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(wh, ww))
        self.qkv = nn.Linear(dim, num_heads * HEAD_DIM * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        _trunc_normal(self.relative_position_bias_table)
        self.softmax = nn.Softmax(dim=-1)

    def fused_kind(self, qkv):
        """None (composed), 'small' (window_attn) or 'large' (window_attn_large) for this call."""
        wh, ww = self.window_size
        if wh != ww or self.dim != self.num_heads * HEAD_DIM:
            return None
        args = (qkv.dtype, qkv.device, HEAD_DIM, self.num_heads, wh, self.relative_position_bias_table)
        p = self.attn_drop.p if self.training else 0.0
        if window_attn.usable_window(*args, dropout_p=p):
            return 'small'
        if window_attn_large.usable_large_window(*args, dropout_p=p):
            return 'large'
        return None

    def forward_map(self, qkv, geometry, kind):
        """qkv (B, Hs*Ws, 3C) of the unshifted map -> (B, Hs*Ws, C) after proj, through the fused kernels."""
        B, L, _ = qkv.shape
        packed = qkv.view(B, L, 3, self.num_heads, HEAD_DIM)
        if kind == 'small':
            out = window_attn.window_attention(packed, self.scale, self.relative_position_bias_table, geometry)
        else:
            out = window_attn_large.large_window_attention(packed, self.scale, self.relative_position_bias_table, geometry)
        return self.proj_drop(self.proj(out))

    def forward(self, x, mask=None):
        return self.attend(self.qkv(x), mask)

    def attend(self, qkv, mask=None):
        """The reference's arithmetic on partitioned windows (:112-137): qkv (B * nW, N, 3C) -> (B * nW, N, C) after proj."""
        B_, N, C3 = qkv.shape
        C = C3 // 3
        q, k, v = qkv.reshape(B_, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
        attn = (q * self.scale) @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, -1)
        attn = attn + bias.permute(2, 0, 1).unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            attn = (attn.view(B_ // nW, nW, self.num_heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, self.num_heads, N, N)
        attn = self.attn_drop(self.softmax(attn))
        x = (attn @ v).transpose(1, 2).reshape(B_, N, C)
        return self.proj_drop(self.proj(x))

    def extra_repr(self):
        return f'dim={self.dim}, window_size={self.window_size}, num_heads={self.num_heads}'


class SwinTransformerBlock(nn.Module):
    """:156-281."""

    def __init__(self, dim, input_resolution, num_heads, window_size=7, shift_size=0, mlp_ratio=4., qkv_bias=True, qk_scale=None,
                 drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.num_heads = num_heads
        self.window_size = window_size
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        if min(self.input_resolution) <= self.window_size:   # the map is one window: no partition, no shift (:185-188)
            self.shift_size = 0
            self.window_size = min(self.input_resolution)
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=_pair(self.window_size), num_heads=num_heads, qkv_bias=qkv_bias,
                                    qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)      # the CLAMPED window (:192-194)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.register_buffer("attn_mask", shift_mask(*input_resolution, self.window_size, self.shift_size)
                             if self.shift_size > 0 else None)

    def forward(self, x):
        H, W = self.input_resolution
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        shortcut = x
        x = self.norm1(x)
        w, shift = self.window_size, self.shift_size
        qkv = self.attn.qkv(x)                               # per token: commutes with the roll and the partition
        kind = self.attn.fused_kind(qkv) if H % w == 0 and W % w == 0 else None
        if kind is not None:
            x = self.attn.forward_map(qkv, (H, W, w, shift, shift), kind)
        else:
            qkv = qkv.view(B, H, W, qkv.shape[-1])
            if shift > 0:
                qkv = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2))
            windows = window_partition(qkv, w).reshape(-1, w * w, qkv.shape[-1])
            x = self.attn.attend(windows, mask=self.attn_mask)
            x = window_reverse(x.view(-1, w, w, C), w, H, W)
            if shift > 0:
                x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
            x = x.reshape(B, H * W, C)
        x = shortcut + self.drop_path(x)
        return x + self.drop_path(self.mlp(self.norm2(x)))

    def extra_repr(self):
        return (f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, "
                f"window_size={self.window_size}, shift_size={self.shift_size}, mlp_ratio={self.mlp_ratio}")


class PatchMerging(nn.Module):
    """:284-330: 2 x 2 neighbours concatenated (order (0,0), (1,0), (0,1), (1,1)), LayerNorm, 4 dim -> out_dim without bias."""

    def __init__(self, input_resolution, dim, out_dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.input_resolution = input_resolution
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, out_dim, bias=False)
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
    """:333-400: `depth` blocks with their own head count, window and MLP ratio; the odd ones shifted and masked."""

    def __init__(self, dim, out_dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4., qkv_bias=True, qk_scale=None,
                 drop=0., attn_drop=0., drop_path=0., norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads[i], window_size=window_size[i],
                                 shift_size=0 if i % 2 == 0 else window_size[i] // 2, mlp_ratio=mlp_ratio[i], qkv_bias=qkv_bias,
                                 qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path, norm_layer=norm_layer)
            for i in range(depth)])
        self.downsample = (downsample(input_resolution, dim=dim, out_dim=out_dim, norm_layer=norm_layer)
                           if downsample is not None else None)

    def forward(self, x):
        for blk in self.blocks:
            if self.use_checkpoint:
                from torch.utils import checkpoint
                x = checkpoint.checkpoint(blk, x)
            else:
                x = blk(x)
        return self.downsample(x) if self.downsample is not None else x

    def extra_repr(self):
        return f"dim={self.dim}, input_resolution={self.input_resolution}, depth={self.depth}"


class SSSTransformer(nn.Module):
    """:451-577."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, num_classes=1000, embed_dim=(96, 192, 384, 768), depths=(2, 2, 6, 2),
                 num_heads=(3, 6, 12, 24), window_size=(7, 7, 7, 7), mlp_ratio=(4., 4., 4., 4.), qkv_bias=True, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 use_checkpoint=False, **kwargs):
        super().__init__()
        self.num_classes = num_classes
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.ape = ape
        self.patch_norm = patch_norm
        self.num_features = int(embed_dim[-1])
        self.mlp_ratio = mlp_ratio
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim[0],
                                      norm_layer=norm_layer if patch_norm else None)
        res = self.patches_resolution = self.patch_embed.patches_resolution
        if ape:
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches, embed_dim[0]))
            _trunc_normal(self.absolute_pos_embed)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = torch.linspace(0, drop_path_rate, sum(depths), device='cpu').tolist()     # host numbers, also under a device context
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            last = i == self.num_layers - 1
            self.layers.append(BasicLayer(
                dim=int(embed_dim[i]), out_dim=None if last else int(embed_dim[i + 1]),
                input_resolution=(res[0] // 2 ** i, res[1] // 2 ** i), depth=depths[i], num_heads=num_heads[i],
                window_size=window_size[i], mlp_ratio=mlp_ratio[i], qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                attn_drop=attn_drop_rate, drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                downsample=None if last else PatchMerging, use_checkpoint=use_checkpoint))
        self.norm = norm_layer(self.num_features)
        self.avgpool = nn.AdaptiveAvgPool1d(1)
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)

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


# the published S3 configurations (AutoFormerV2/configs/S3-{T,S,B}.yaml): stage 3 always has 14 x 14 windows, S3-S every stage;
# every block of a stage has the same head count, window and MLP ratio
_DEPTHS = dict(T=[2, 2, 6, 2], S=[2, 2, 18, 2], B=[2, 2, 30, 2])
_WINDOWS = dict(T=[7, 7, 14, 7], S=[14, 14, 14, 14], B=[7, 7, 14, 7])


def s3_config(size='T'):
    """Constructor arguments of S3-{T,S,B} as the per-stage, per-block lists the model takes."""
    depths = _DEPTHS[size]
    per_block = lambda vals: [[v] * d for v, d in zip(vals, depths)]          # noqa: E731
    return dict(embed_dim=[96, 192, 384, 768], depths=list(depths), num_heads=per_block([3, 6, 12, 24]),
                window_size=per_block(_WINDOWS[size]), mlp_ratio=per_block([4.0, 4.0, 4.0, 4.0]))


def s3(size='T', img_size=224, **kwargs):
    """S3-T / S3-S / S3-B at 224 with patch 4."""
    kw = dict(img_size=img_size, patch_size=4, **s3_config(size))
    kw.update(kwargs)
    return SSSTransformer(**kw)


@torch.no_grad()
def evaluate(model, loader, device, amp=True):
    """Mirror of `evaluate` in AutoFormerV2/engine.py:14-46 with bf16 autocast where the reference uses fp16: eval mode, cross
    entropy averaged over the batches, top-1 / top-5 accuracy (per cent) averaged over the samples.  -> {'loss', 'acc1',
    'acc5'}.  The statistics are accumulated on the device: one host synchronisation at the end."""
    model.eval()
    device = torch.device(device)
    tot = torch.zeros(3, dtype=torch.float64, device=device)     # sum of the batch losses, top-1 hits, top-5 hits
    batches = samples = 0
    for images, target in loader:
        images = images.to(device, non_blocking=True)
        target = target.to(device, non_blocking=True)
        with torch.autocast(device_type=device.type, dtype=torch.bfloat16, enabled=amp and device.type == 'cuda'):
            output = model(images)
            loss = F.cross_entropy(output, target)
        top5 = output.float().topk(min(5, output.shape[1]), dim=1).indices
        hit = top5.eq(target.view(-1, 1))
        tot += torch.stack([loss.double(), hit[:, 0].sum().double(), hit.any(dim=1).sum().double()])
        batches += 1
        samples += images.shape[0]
    loss, top1, top5 = tot.tolist()
    return {'loss': loss / max(batches, 1), 'acc1': 100.0 * top1 / max(samples, 1), 'acc5': 100.0 * top5 / max(samples, 1)}
