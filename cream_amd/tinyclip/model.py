"""TinyCLIP's two towers — host-side mirror of TinyCLIP/src/open_clip/model.py, for the dense models of the manual
weight-inheritance recipe and the masked ones of the automatic recipe: `ResidualAttentionBlock` :208-315, `Transformer`
:342-427, `VisualTransformer` :442-543, `ImageEncoder` :597-675, `TextEncoder` :682-818, `LogitScale` :847-853, `CLIPBase` /
`CLIP` :874-1112.

Same constructor configuration (the JSON files of open_clip/model_configs), parameter names and state-dict keys
(`_image_encoder.visual.transformer.resblocks.{i}.attn.in_proj_weight`, `_text_encoder.token_embedding.weight`,
`_logit_scale.logit_scale`, ...), so TinyCLIP / OpenCLIP checkpoints in the reference's "new" layout load.

What is different is the execution: the towers run batch-first (the reference permutes to sequence-first for
`nn.MultiheadAttention` and back), and the attention core of a block whose heads are 64 wide runs — under bf16 autocast
on the device — on the fused flash-style kernels of csrc/irpe_attn.hip (`irpe_fused.attention` without any relative
position term: nothing of size L^2 reaches HBM, forward one launch, backward two).  Under bf16 autocast on the device the
whole run of blocks of a tower — image AND text (causal mask inside the attention kernels) — is one autograd node on the
own GEMM / LayerNorm / attention kernels (cream_amd.tinyclip.native); every fp32 / CPU call uses the composed form.

The learnable pruning masks of the automatic weight inheritance (`l0module.py` -> cream_amd.tinyclip.l0) are mirrored too:
every forward takes the reference's mask arguments (`hidden_z`, `heads_z`, `mha_z`, `intermediate_z`, `ffn_z`, `embed_dim_z`),
the encoders take `l0_module_image` / `l0_module_text` + `mask_cfg` and draw their masks from `self.l0_module.forward()`
(:659-675, :810-818), and `prune()` folds the masks into the weights and cuts the modules down, literally as the reference
does — including its asymmetry: `proj` / `text_projection` rows are multiplied by `hidden_z` (:561-565, :842-843) although
the forward does not multiply the final LayerNorm's output, so "pruned == masked" holds for 0/1 masks only.  With every mask
None each class runs exactly the code of the dense recipe, and the dense state-dict keys are unchanged.  The composed masked
form (the reference's formulation, batch-first) serves fp32, CPU, QuickGELU towers and any call with `mha_z` / `ffn_z`; a tower
cut by `prune()` runs without masks, under bf16 autocast on the device as one node on zero-padded operands
(cream_amd.tinyclip.native_pruned); under bf16 autocast on the device a tower with `hidden_z` / `heads_z` / `intermediate_z` is one autograd node with
the masks folded into the operands (cream_amd.tinyclip.native_masked, csrc/l0_mask.hip).

Not mirrored: `weight_inherit.py`'s manual inheritance, the ResNet / timm image towers, gradient checkpointing.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import os

from .. import irpe_fused

NATIVE_TOWERS = os.environ.get('CREAM_TINYCLIP_NATIVE', '1') != '0'     # image towers on cream_amd.tinyclip.native


def _kept(z):
    return torch.where(z != 0)[0]


class LayerNorm(nn.LayerNorm):
    """model.py:40-99 (torch's layer_norm handles low-precision inputs under autocast).  With `hidden_z` (C,): the masked
    LayerNorm — statistics over the columns with hidden_z != 0 only, exact zeros elsewhere, no gradient into hidden_z."""
    hidden_z = None

    def forward(self, x, hidden_z=None):
        self.hidden_z = hidden_z
        if hidden_z is None:
            return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps).to(x.dtype)
        assert len(self.normalized_shape) == 1
        idx = _kept(hidden_z)
        normed = F.layer_norm(torch.index_select(x, -1, idx), [len(idx)], self.weight[idx], self.bias[idx], self.eps)
        out = x.new_zeros(x.shape)
        out[..., idx] = normed.to(x.dtype)
        return out

    def prune(self):                                            # model.py:70-83
        if self.hidden_z is None:
            return self
        idx = _kept(self.hidden_z)
        m = LayerNorm(idx.shape[0]).to(self.weight.device)
        m.eps = self.eps
        m.weight.data = self.weight[idx].contiguous()
        m.bias.data = self.bias[idx].contiguous()
        return m


class QuickGELU(nn.Module):
    def forward(self, x):                                       # model.py:102-105
        return x * torch.sigmoid(1.702 * x)


class Mlp(nn.Module):
    def __init__(self, d_model, mlp_width, act_layer=nn.GELU):   # model.py:108-137
        super().__init__()
        self.c_fc = nn.Linear(d_model, mlp_width)
        self.gelu = act_layer()
        self.c_proj = nn.Linear(mlp_width, d_model)

    hidden_z = intermediate_z = None

    def forward(self, x, hidden_z=None, intermediate_z=None):
        """hidden_z (d_model,) / intermediate_z (mlp_width,), or broadcastable to (N, L, .)."""
        self.hidden_z, self.intermediate_z = hidden_z, intermediate_z
        x = self.gelu(self.c_fc(x))
        if intermediate_z is not None:
            x = torch.mul(x, intermediate_z)
        x = self.c_proj(x)
        if hidden_z is not None:
            x = torch.mul(x, hidden_z)
        return x

    def prune(self):                                            # model.py:139-166: the masks folded into c_proj, then cut
        dev = self.c_fc.weight.device
        D, F_ = self.c_fc.weight.shape[1], self.c_fc.weight.shape[0]
        zh = self.hidden_z if self.hidden_z is not None else torch.ones(D, dtype=torch.bool, device=dev)
        zi = self.intermediate_z if self.intermediate_z is not None else torch.ones(F_, dtype=torch.bool, device=dev)
        hr, ir = _kept(zh.reshape(-1)), _kept(zi.reshape(-1))
        m = Mlp.__new__(Mlp)
        nn.Module.__init__(m)
        m.c_fc, m.gelu, m.c_proj = nn.Linear(len(hr), len(ir), device=dev), self.gelu, nn.Linear(len(ir), len(hr), device=dev)
        m.c_fc.weight = nn.Parameter(self.c_fc.weight[ir][:, hr].contiguous())
        m.c_fc.bias = nn.Parameter(self.c_fc.bias[ir].contiguous())
        m.c_proj.weight = nn.Parameter((self.c_proj.weight * zi.view(1, -1) * zh.view(-1, 1))[hr][:, ir].contiguous())
        m.c_proj.bias = nn.Parameter((self.c_proj.bias * zh.reshape(-1))[hr].contiguous())
        return m


class MultiheadAttention(nn.Module):
    """The parameters of `nn.MultiheadAttention(d_model, n_head)` (packed `in_proj_weight` / `in_proj_bias`, `out_proj`)
    with a batch-first self-attention forward."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        assert embed_dim % num_heads == 0
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.)

    head_z = hidden_z = None

    def forward(self, x, attn_mask=None, head_z=None, hidden_z=None):
        """x (N, L, D); attn_mask additive (L, L) or None; head_z (H,) scales each head's output before the output
        projection, hidden_z (D,) the projection's output (model.py:250-283, batch-first; the fused attention core stays:
        nothing of size L^2 is written for the masks' sake).  A pruned module has H * head_dim != D."""
        self.head_z, self.hidden_z = head_z, hidden_z
        N, L, _ = x.shape
        H, hd = self.num_heads, self.head_dim
        qkv = F.linear(x, self.in_proj_weight, self.in_proj_bias)
        if attn_mask is None and irpe_fused.usable(qkv.dtype, qkv.device, hd, L, (None, None, None), False):
            out = irpe_fused.attention(qkv.view(N, L, 3, H, hd), hd ** -0.5, None, None, None)       # (N, L, H * hd)
        else:
            q, k, v = qkv.view(N, L, 3, H, hd).permute(2, 0, 3, 1, 4).unbind(0)                        # (N, H, L, hd)
            attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
            if attn_mask is not None:
                attn = attn + attn_mask.to(attn.dtype)
            out = (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(N, L, H * hd)
        if head_z is not None:
            out = (out.reshape(N, L, H, hd) * head_z.view(1, 1, H, 1)).reshape(N, L, H * hd)
        out = self.out_proj(out)
        if hidden_z is not None:
            out = torch.mul(out, hidden_z)
        return out

    def prune(self):                                            # model.py:170-205 (in place, as there)
        dev = self.in_proj_weight.device
        H0, hd, D0 = self.num_heads, self.head_dim, self.in_proj_weight.shape[1]
        zh = self.hidden_z if self.hidden_z is not None else torch.ones(D0, dtype=torch.bool, device=dev)
        zd = self.head_z if self.head_z is not None else torch.ones(H0, dtype=torch.bool, device=dev)
        zh, zd = zh.reshape(-1), zd.reshape(-1)
        hr, dr = _kept(zh), _kept(zd)
        d_model, d_head = len(hr), len(dr)
        wo = ((self.out_proj.weight * zh.view(-1, 1)).view(D0, H0, hd) * zd.view(1, H0, 1))[hr][:, dr].reshape(d_model, -1)
        bo = (self.out_proj.bias * zh)[hr].reshape(-1)
        self.in_proj_weight = nn.Parameter(self.in_proj_weight.view(3, H0, hd, D0)[:, dr][..., hr].reshape(-1, d_model))
        self.in_proj_bias = nn.Parameter(self.in_proj_bias.view(3, H0, hd)[:, dr].reshape(-1))
        self.out_proj.weight, self.out_proj.bias = nn.Parameter(wo), nn.Parameter(bo)
        self.embed_dim, self.num_heads = d_model, d_head
        return self


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model, n_head, mlp_ratio=4.0, act_layer=nn.GELU):      # model.py:208-236
        super().__init__()
        self.ln_1 = LayerNorm(d_model)
        self.attn = MultiheadAttention(d_model, n_head)
        self.ln_attn = nn.Identity()
        self.ln_2 = LayerNorm(d_model)
        self.mlp = Mlp(d_model, int(d_model * mlp_ratio), act_layer)

    hidden_z = heads_z = mha_z = intermediate_z = ffn_z = None

    def forward(self, x, attn_mask=None, hidden_z=None, heads_z=None, mha_z=None, intermediate_z=None, ffn_z=None):
        """model.py:285-315.  A pruned block may have lost its attention or its MLP branch (`attn` / `mlp` is None)."""
        self.hidden_z, self.heads_z, self.mha_z, self.intermediate_z, self.ffn_z = hidden_z, heads_z, mha_z, intermediate_z, ffn_z
        if self.attn is not None:
            a = self.attn(self.ln_1(x, hidden_z), attn_mask, heads_z, hidden_z)
            if mha_z is not None:                               # a number
                a = a.mul(mha_z)
            x = x + a
        if self.mlp is not None:
            m = self.mlp(self.ln_2(x, hidden_z), hidden_z, intermediate_z)
            if ffn_z is not None:                               # a number
                m = m.mul(ffn_z)
            x = x + m
        return x

    def prune(self):                                            # model.py:317-339 (in place)
        if (self.mha_z is not None and self.mha_z.item() == 0) or (self.heads_z is not None and self.heads_z.sum() == 0):
            self.ln_1 = self.attn = None
        else:
            self.ln_1, self.attn = self.ln_1.prune(), self.attn.prune()
            if self.mha_z is not None:
                self.attn.out_proj.weight.data *= self.mha_z
                self.attn.out_proj.bias.data *= self.mha_z
        if self.ffn_z is not None and self.ffn_z.item() == 0:
            self.ln_2 = self.mlp = None
        else:
            self.ln_2, self.mlp = self.ln_2.prune(), self.mlp.prune()
            if self.ffn_z is not None:
                self.mlp.c_proj.weight.data *= self.ffn_z
                self.mlp.c_proj.bias.data *= self.ffn_z
        return self


class Transformer(nn.Module):
    def __init__(self, width, layers, heads, mlp_ratio=4.0, act_layer=nn.GELU):  # model.py:342-359
        super().__init__()
        self.width, self.layers, self.num_heads, self.head_dim, self.mlp_ratio = width, layers, heads, width // heads, mlp_ratio
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads, mlp_ratio, act_layer) for _ in range(layers)])

    def forward(self, x, attn_mask=None, causal=False, hidden_z=None, heads_z=None, mha_z=None, intermediate_z=None, ffn_z=None):
        """`causal=True`: the caller states that attn_mask is the upper-triangular -inf mask (the text tower's buffer).
        The masks are L0Module's (model.py:375-424): hidden_z (width,), heads_z (layers, 1, heads, 1, 1) / (layers, heads) /
        (heads,), intermediate_z (layers, 1, 1, 4 width) / (layers, 4 width) / (4 width,), mha_z / ffn_z (layers,)."""
        if hidden_z is None and heads_z is None and mha_z is None and intermediate_z is None and ffn_z is None:
            if x.is_cuda and NATIVE_TOWERS:
                from . import native
                if native.supported(self, x, attn_mask, causal):   # bf16 autocast, heads of 64: the own kernels end to end
                    return native.tower(self, x, causal and attn_mask is not None)
                from . import native_pruned
                if native_pruned.supported(self, x, attn_mask, causal):   # a tower cut by prune(): the same node on padded operands
                    return native_pruned.tower(self, x, causal and attn_mask is not None)
            for blk in self.resblocks:
                x = blk(x, attn_mask)
            return x
        n = self.layers
        if hidden_z is not None:
            assert hidden_z.shape == (self.width,), hidden_z.shape
        if heads_z is not None:
            if heads_z.ndim == 5:
                heads_z = heads_z.view(n, self.num_heads)
            assert heads_z.shape in [(n, self.num_heads), (self.num_heads,)], (heads_z.shape, (n, self.num_heads))
        if mha_z is not None:
            assert mha_z.shape == (n,), mha_z.shape
        if intermediate_z is not None:
            if intermediate_z.ndim == 4:
                intermediate_z = intermediate_z.view(n, -1)
            assert intermediate_z.shape in [(n, self.mlp_ratio * self.width), (self.mlp_ratio * self.width,)], intermediate_z.shape
        if ffn_z is not None:
            assert ffn_z.shape == (n,), ffn_z.shape

        def zi(z, i, ndim=2):
            return z[i] if z is not None and z.ndim == ndim else z

        if x.is_cuda and NATIVE_TOWERS and mha_z is None and ffn_z is None:
            from . import native_masked
            if native_masked.supported(self, x, attn_mask, causal, hidden_z, heads_z, intermediate_z):
                return native_masked.tower(self, x, causal and attn_mask is not None, hidden_z, heads_z, intermediate_z)
        for i, blk in enumerate(self.resblocks):
            x = blk(x, attn_mask, hidden_z, zi(heads_z, i), zi(mha_z, i, 1), zi(intermediate_z, i), zi(ffn_z, i, 1))
        return x

    def prune(self):                                            # model.py:435-439
        for i in range(len(self.resblocks)):
            self.resblocks[i] = self.resblocks[i].prune()
        return self


class VisualTransformer(nn.Module):
    def __init__(self, image_size, patch_size, width, layers, heads, mlp_ratio, output_dim, act_layer=nn.GELU):
        super().__init__()                                                      # model.py:442-482
        self.image_size, self.patch_size = (image_size, image_size), (patch_size, patch_size)
        self.grid_size = (image_size // patch_size, image_size // patch_size)
        self.output_dim, self.embed_dim, self.layers, self.head_dim = output_dim, width, layers, width // heads
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.grid_size[0] * self.grid_size[1] + 1, width))
        self.ln_pre = LayerNorm(width)
        self.transformer = Transformer(width, layers, heads, mlp_ratio, act_layer=act_layer)
        self.ln_post = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))

    def patches(self, x):
        """`conv1` (kernel = stride = patch, no bias, model.py:462-463,503-507) as ONE GEMM over the unfolded patches:
        (N * grid^2, 3 * p * p) x (3 * p * p, width).  Against the framework's convolution route (which first spends its
        warm-up steps searching, naive kernels included) the steady-state step is 1 % faster (same-box A/B, 81.0 -> 80.3 ms)."""
        N, C, Hh, Ww = x.shape
        p = self.patch_size[0]
        gh, gw = Hh // p, Ww // p
        x = x.reshape(N, C, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(N, gh * gw, C * p * p)
        return F.linear(x, self.conv1.weight.reshape(self.conv1.weight.shape[0], -1))

    hidden_z = embed_dim_z = None

    def forward(self, x, hidden_z=None, heads_z=None, mha_z=None, intermediate_z=None, ffn_z=None, embed_dim_z=None):
        self.hidden_z, self.embed_dim_z = hidden_z, embed_dim_z                 # model.py:493-535
        x = self.patches(x)                                                     # (N, grid^2, width)
        cls = self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding.to(x.dtype)
        if hidden_z is not None:
            x = torch.mul(x, hidden_z)
        x = self.transformer(self.ln_pre(x, hidden_z), hidden_z=hidden_z, heads_z=heads_z, mha_z=mha_z,
                             intermediate_z=intermediate_z, ffn_z=ffn_z)
        return self.ln_post(x[:, 0, :], hidden_z) @ self.proj

    def prune(self):
        """model.py:545-566, literally — `proj`'s rows are multiplied by hidden_z although the forward does not multiply
        ln_post's output: pruned == masked for 0/1 masks only."""
        zh = self.hidden_z
        hr = _kept(zh)
        self.conv1.weight = nn.Parameter((self.conv1.weight.data * zh.view(-1, 1, 1, 1))[hr])
        self.class_embedding = nn.Parameter((self.class_embedding * zh.view(-1))[hr])
        self.positional_embedding = nn.Parameter((self.positional_embedding * zh.view(1, -1))[:, hr])
        self.ln_pre = self.ln_pre.prune()
        self.transformer = self.transformer.prune()
        self.ln_post = self.ln_post.prune()
        if self.embed_dim_z is not None:
            self.proj = nn.Parameter((self.proj * zh.view(-1, 1) * self.embed_dim_z.view(1, -1))[hr][:, self.embed_dim_z > 0])
        else:
            self.proj = nn.Parameter((self.proj * zh.view(-1, 1))[hr])
        return self


def _l0_module(width, heads, layers, mask_cfg):
    """The L0Module of a tower (model.py:638-649, :720-731): `mask_cfg` has sparsity_warmup / sparsity / start_sparsity as
    attributes or keys."""
    from types import SimpleNamespace
    from .l0 import L0Module
    get = (lambda k: mask_cfg[k]) if isinstance(mask_cfg, dict) else (lambda k: getattr(mask_cfg, k))
    cfg = SimpleNamespace(hidden_size=width, intermediate_size=4 * width, num_attention_heads=heads, num_hidden_layers=layers)
    return L0Module(cfg, lagrangian_warmup=get("sparsity_warmup"), start_sparsity=get("start_sparsity"),
                    target_sparsity=get("sparsity"), pruning_type=["hidden", "heads", "intermediate"])


def _l0_masks(enc):
    """`enc.l0_module.forward()` (model.py:662-663, :813-814).  In eval mode the masks are a function of the l0 parameters
    alone: they are kept until a parameter's version (or storage) changes, so the same tensors come back and the operand
    pack of cream_amd.tinyclip.native_masked — keyed on the masks' versions — is reused across forwards."""
    l0 = enc.l0_module
    if l0.training:
        return l0.forward()
    key = tuple((p.data_ptr(), p._version) for p in l0.parameters())
    cached = enc.__dict__.get("_l0_eval_masks")
    if cached is None or cached[0] != key:
        cached = enc.__dict__["_l0_eval_masks"] = (key, l0.forward())
    return dict(cached[1])


class ImageEncoder(nn.Module):
    def __init__(self, embed_dim, vision_cfg, quick_gelu, l0_module_image=False, mask_cfg=None):   # model.py:597-653 (ViT branch)
        super().__init__()
        c = dict(layers=12, width=768, head_width=64, mlp_ratio=4.0, patch_size=16, image_size=224)
        c.update(vision_cfg)
        if c.get("timm_model_name") or isinstance(c["layers"], (tuple, list)):
            raise NotImplementedError("ImageEncoder: only the ViT tower is on this path (model.py:603-622 are the timm / ResNet towers)")
        self.visual = VisualTransformer(c["image_size"], c["patch_size"], c["width"], c["layers"], c["width"] // c["head_width"],
                                        c["mlp_ratio"], embed_dim, act_layer=QuickGELU if quick_gelu else nn.GELU)
        self.l0_module = _l0_module(c["width"], c["width"] // c["head_width"], c["layers"], mask_cfg) if l0_module_image else None
        self.mask = None

    def forward(self, image, normalized=False, **mask):                         # model.py:659-675
        if self.l0_module is not None:
            mask = _l0_masks(self)
        self.mask = mask
        f = self.visual(image, **mask)
        if mask.get("embed_dim_z") is not None:
            f = f.mul(mask["embed_dim_z"])
        return F.normalize(f, dim=-1) if normalized else f

    def prune(self):
        self.visual = self.visual.prune()
        return self


class TextEncoder(nn.Module):
    hidden_z = embed_dim_z = None

    def __init__(self, embed_dim, text_cfg, quick_gelu, l0_module_text=False, mask_cfg=None):      # model.py:682-735
        super().__init__()
        c = dict(context_length=77, vocab_size=49408, width=512, heads=8, layers=12)
        c.update(text_cfg)
        self.context_length, self.vocab_size = c["context_length"], c["vocab_size"]
        self.transformer = Transformer(c["width"], c["layers"], c["heads"], act_layer=QuickGELU if quick_gelu else nn.GELU)
        self.token_embedding = nn.Embedding(c["vocab_size"], c["width"])
        self.positional_embedding = nn.Parameter(torch.empty(self.context_length, c["width"]))
        self.ln_final = LayerNorm(c["width"])
        self.text_projection = nn.Parameter(torch.empty(c["width"], embed_dim))
        self.register_buffer("attn_mask", self.build_attention_mask(), persistent=False)
        self.init_parameters()
        self.l0_module = _l0_module(c["width"], c["heads"], c["layers"], mask_cfg) if l0_module_text else None
        self.mask = None

    def init_parameters(self):                                                  # model.py:737-754
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        t = self.transformer
        proj_std, attn_std, fc_std = (t.width ** -0.5) * ((2 * t.layers) ** -0.5), t.width ** -0.5, (2 * t.width) ** -0.5
        for blk in t.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(blk.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(blk.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(blk.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=t.width ** -0.5)

    def build_attention_mask(self):                                             # model.py:756-762 (causal, additive)
        return torch.full((self.context_length, self.context_length), float("-inf")).triu_(1)

    def encode_text(self, text, normalized=False, hidden_z=None, heads_z=None, mha_z=None, intermediate_z=None, ffn_z=None,
                    embed_dim_z=None):                                          # model.py:764-805
        self.hidden_z, self.embed_dim_z = hidden_z, embed_dim_z
        x = self.token_embedding(text) + self.positional_embedding
        if hidden_z is not None:
            x = torch.mul(x, hidden_z)
        x = self.transformer(x, attn_mask=self.attn_mask[:x.shape[1], :x.shape[1]], causal=True, hidden_z=hidden_z, heads_z=heads_z,
                             mha_z=mha_z, intermediate_z=intermediate_z, ffn_z=ffn_z)
        x = self.ln_final(x, hidden_z)
        x = x[torch.arange(x.shape[0], device=x.device), text.argmax(dim=-1)] @ self.text_projection   # the eot token
        if embed_dim_z is not None:
            x = x.mul(embed_dim_z)
        return F.normalize(x, dim=-1) if normalized else x

    def forward(self, text, normalized=False):                                  # model.py:810-818
        mask = _l0_masks(self) if self.l0_module is not None else dict()
        self.mask = mask
        return self.encode_text(text, normalized=normalized, **mask)

    def prune(self):
        """model.py:820-844, literally (`text_projection`'s rows times hidden_z, see VisualTransformer.prune)."""
        dev = self.token_embedding.weight.device
        zh = self.hidden_z if self.hidden_z is not None else torch.ones(self.text_projection.size(0), device=dev)
        ze = self.embed_dim_z if self.embed_dim_z is not None else torch.ones(self.text_projection.size(1), device=dev)
        hr, er = zh > 0, ze > 0
        tok = (self.token_embedding.weight * zh.view(1, -1))[:, hr]
        self.token_embedding = nn.Embedding(tok.shape[0], tok.shape[1], device=dev)
        self.token_embedding.weight = nn.Parameter(tok)
        self.positional_embedding = nn.Parameter((self.positional_embedding * zh.view(1, -1))[:, hr])
        self.transformer = self.transformer.prune()
        self.ln_final = self.ln_final.prune()
        self.text_projection = nn.Parameter((self.text_projection * zh.view(-1, 1) * ze.view(1, -1))[hr][:, er])
        return self


class LogitScale(nn.Module):
    def __init__(self):                                                         # model.py:847-853
        super().__init__()
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))

    def forward(self, dummy=None):
        return self.logit_scale


class CLIP(nn.Module):
    """model.py:874-1112: `forward(image, text, normalized=True)` -> (image features, text features, exp(logit scale));
    a tower whose input is None is skipped (:990-1001)."""

    def __init__(self, embed_dim, vision_cfg, text_cfg, quick_gelu=False, mask_image=False, mask_text=False, sparsity_warmup=1000,
                 sparsity=0.25, start_sparsity=0.0, mask_cfg=None):
        super().__init__()
        if mask_cfg is None:                                                    # model.py:1098-1101
            mask_cfg = dict(sparsity_warmup=sparsity_warmup, sparsity=sparsity, start_sparsity=start_sparsity)
        self._image_encoder = ImageEncoder(embed_dim, vision_cfg, quick_gelu, l0_module_image=mask_image, mask_cfg=mask_cfg)
        self._text_encoder = TextEncoder(embed_dim, text_cfg, quick_gelu, l0_module_text=mask_text, mask_cfg=mask_cfg)
        self._logit_scale = LogitScale()
        # per-tower precision (model.py:883-896; train.py:91-99 passes get_autocast(args.image_precision / text_precision /
        # logit_precision)): context-manager FACTORIES, entered around each tower
        from contextlib import nullcontext
        self.image_autocast = self.text_autocast = self.logit_autocast = nullcontext

    def set_autocast(self, image_autocast, text_autocast, logit_autocast):      # model.py:893-896
        self.image_autocast, self.text_autocast, self.logit_autocast = image_autocast, text_autocast, logit_autocast

    visual = property(lambda self: self._image_encoder.visual)
    transformer = property(lambda self: self._text_encoder.transformer)
    logit_scale = property(lambda self: self._logit_scale.logit_scale)

    def encode_image(self, image, normalized=False):                            # model.py:1003-1005
        with self.image_autocast():
            return self._image_encoder(image, normalized=normalized)

    def encode_text(self, text, normalized=False):                              # model.py:1007-1009
        with self.text_autocast():
            return self._text_encoder(text, normalized=normalized)

    def forward(self, image, text, normalized=True):                            # model.py:990-1001
        fi = ft = None
        if image is not None:
            with self.image_autocast():
                fi = self._image_encoder(image, normalized=normalized)
        if text is not None:
            with self.text_autocast():
                ft = self._text_encoder(text, normalized=normalized)
        with self.logit_autocast():
            scale = self._logit_scale()
        return fi, ft, scale.exp()

    def load_state_dict(self, state_dict, strict=True):                         # model.py:1049-1070
        return super().load_state_dict(convert_to_new_checkpoint(state_dict), strict=strict)

    def lock_image_tower(self):                                                 # model.py:1015-1021
        for p in self._image_encoder.parameters():
            p.requires_grad = False

    def lock_text_tower(self):
        for p in self._text_encoder.parameters():
            p.requires_grad = False


def convert_to_new_checkpoint(state_dict):
    """Any of the layouts TinyCLIP / OpenCLIP checkpoints come in -> the `_image_encoder. / _text_encoder. /
    _logit_scale.` layout of this class (model.py:1115-1157 with `used_ddp=False`, plus the `.module` strip of
    `CLIPBase.load_state_dict`, :1066-1070):
      * the new layout saved from DDP-wrapped towers (`_image_encoder.module.visual...`): the `module` level is removed;
      * the old single-module layout (`visual.*`, `logit_scale`, text keys at the root), optionally under `module.`."""
    if '_logit_scale.module.logit_scale' in state_dict:
        out = {}
        for k, v in state_dict.items():
            sp = k.split('.')
            assert sp[1] == 'module', k
            out['.'.join(sp[:1] + sp[2:])] = v
        return out
    if '_logit_scale.logit_scale' in state_dict:
        return dict(state_dict)
    if 'module.logit_scale' in state_dict:
        state_dict = {k[len('module.'):]: v for k, v in state_dict.items()}
    if 'logit_scale' not in state_dict:
        return dict(state_dict)
    out = {}
    for k, v in state_dict.items():
        if k.startswith('visual.'):
            out['_image_encoder.' + k] = v
        elif k == 'logit_scale':
            out['_logit_scale.logit_scale'] = v
        else:
            out['_text_encoder.' + k] = v
    return out


# open_clip/model_configs/*.json of the configurations BASELINE config 5 names
MODEL_CONFIGS = OrderedDict([
    ("TinyCLIP-ViT-39M-16-Text-19M", dict(embed_dim=512, vision_cfg=dict(image_size=224, layers=12, width=512, patch_size=16),
                                          text_cfg=dict(context_length=77, vocab_size=49408, width=512, heads=8, layers=6))),
    ("ViT-B-16", dict(embed_dim=512, vision_cfg=dict(image_size=224, layers=12, width=768, patch_size=16),
                      text_cfg=dict(context_length=77, vocab_size=49408, width=512, heads=8, layers=12))),
])


def create_model(name, **overrides):
    """factory.py `create_model` for the two configurations above (no pretrained download: there is no network).
    `mask_image=True` / `mask_text=True` with `mask_cfg=dict(sparsity_warmup=, sparsity=, start_sparsity=)` give the towers their
    `l0_module` (factory.py:131-132)."""
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in MODEL_CONFIGS[name].items()}
    for k, v in overrides.items():
        if isinstance(v, dict) and isinstance(cfg.get(k), dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    return CLIP(**cfg)


def n_params(m):
    return sum(p.numel() for p in m.parameters())


__all__ = ["CLIP", "Mlp", "MultiheadAttention", "ImageEncoder", "TextEncoder", "VisualTransformer", "Transformer", "ResidualAttentionBlock", "LayerNorm",
           "QuickGELU", "MODEL_CONFIGS", "create_model", "n_params", "convert_to_new_checkpoint"]
