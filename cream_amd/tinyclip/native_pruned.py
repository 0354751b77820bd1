"""Pruned TinyCLIP towers on the framework's own kernels — the node of cream_amd.tinyclip.native for a tower cut by
`prune()` (TinyCLIP/src/open_clip/model.py:139-205, :317-339; every published TinyCLIP-auto-* student is one): the stream is
d = len(kept hidden) columns wide, any integer; inner_l = 64 H_l and the MLP width F_l differ per layer; a block may have lost
its attention branch, its MLP branch, or both.

A pruned tower is the DENSE node run on ZERO-PADDED operands: Dp = d and Fp_l = F_l rounded up to the GEMM granularity
(pruned_ops.GRANULE = 8: what the NT, NT + GELU, dgrad, dgrad x gelu' and TN weight-gradient products all accept; inner_l
needs none).  The padding columns of every activation are exact zeros by construction — zero rows of W_o / W_2 and zero bias
entries, zero rows of W_1 (gelu(0) = 0), zero rows of W_2^T under gelu'(0) = 1/2, and the masked LayerNorm of csrc/l0_mask.hip
run with the mask [1] * d + [0] * (Dp - d): statistics over d columns, exact zeros elsewhere.  Parameters, `.grad`, optimizer
state and the state dict stay in the reference's compact shapes:

  * the padded bf16 W / W^T / bias copies are allocated once as zeros and filled by the existing copy launch
    (cream_adamw_step's copy mode: rows, cols compact, ld_mir padded), the padded fp32 gamma / beta by cream_pad_cols;
  * the stream enters through cream_pad_cols ((M, d) any float dtype -> (M, Dp) fp32) and leaves through cream_unpad_cols;
  * the split-K partials of the weight gradients, laid out on the padded shapes, are added into the compact `.grad` by
    cream_grad_finalize_compact on the weight-gradient stream (the summation tree of cream_grad_finalize, bit for bit).

The tower is a chain of HALVES (LayerNorm -> branch -> pending residual add), one per branch a block still has; a block with
neither is the identity and contributes nothing.  The residual add of a half is folded into the LayerNorm of the next one, as
in the dense node, whichever block that belongs to.  n_keep = d comes from the shapes: no host synchronisation.

Not here (composed path): QuickGELU towers, fp32, CPU, masks (cream_amd.tinyclip.native_masked), gradient checkpointing.
"""
import torch

from .. import irpe_fused
from ..autoformer import block as K
from . import mask_ops as MO
from . import native
from . import pruned_ops as P

_OPS_KEY = '_cream_tc_pruned_operands'
MAX_STREAM = 1280       # the LayerNorm kernels' widest row (csrc/l0_mask.hip: LN_MAXC)


def _attn_shapes_ok(blk, d):
    at, ln = blk.attn, blk.ln_1
    H = at.num_heads
    inner = 64 * H
    return (H >= 1 and at.head_dim == 64 and ln is not None and tuple(ln.weight.shape) == (d,) and tuple(ln.bias.shape) == (d,)
            and tuple(at.in_proj_weight.shape) == (3 * inner, d) and tuple(at.in_proj_bias.shape) == (3 * inner,)
            and tuple(at.out_proj.weight.shape) == (d, inner) and tuple(at.out_proj.bias.shape) == (d,))


def _mlp_shapes_ok(blk, d):
    mlp, ln = blk.mlp, blk.ln_2
    F_ = mlp.c_fc.weight.shape[0]
    return (F_ >= 1 and ln is not None and tuple(ln.weight.shape) == (d,) and tuple(ln.bias.shape) == (d,)
            and tuple(mlp.c_fc.weight.shape) == (F_, d) and tuple(mlp.c_fc.bias.shape) == (F_,)
            and tuple(mlp.c_proj.weight.shape) == (d, F_) and tuple(mlp.c_proj.bias.shape) == (d,))


def plan(transformer, d=None):
    """-> dict(d, Dp, blocks=[dict(attn, mlp, H, F, Fp)]) from the parameter shapes alone, or None when they are not those
    of one pruned tower.  `d`: the stream width of the input (x.shape[-1]); without it the first remaining projection
    decides (`transformer.width` keeps its pre-prune value).  A tower that has lost every branch has no width of its own."""
    blocks = []
    for blk in transformer.resblocks:
        has_attn, has_mlp = getattr(blk, 'attn', None) is not None, getattr(blk, 'mlp', None) is not None
        if d is None and has_attn:
            d = blk.attn.in_proj_weight.shape[1]
        if d is None and has_mlp:
            d = blk.mlp.c_fc.weight.shape[1]
        if (has_attn and not _attn_shapes_ok(blk, d)) or (has_mlp and not _mlp_shapes_ok(blk, d)):
            return None
        F_ = blk.mlp.c_fc.weight.shape[0] if has_mlp else 0
        blocks.append(dict(attn=has_attn, mlp=has_mlp, H=blk.attn.num_heads if has_attn else 0, F=F_, Fp=P.padded(F_)))
    if d is None or d < 1:
        return None
    return dict(d=d, Dp=P.padded(d), blocks=blocks)


def _block_supported(blk):
    """native._block_supported for a block that may have lost a branch: erf-GELU, ln_attn identity, fp32 parameters."""
    if not isinstance(getattr(blk, 'ln_attn', None), torch.nn.Identity):
        return False
    if blk.mlp is not None and not (isinstance(blk.mlp.gelu, torch.nn.GELU) and getattr(blk.mlp.gelu, 'approximate', 'none') == 'none'):
        return False
    return all(p.dtype == torch.float32 for p in blk.parameters())


def supported(transformer, x, attn_mask, causal=False):
    """The environment and parameter conditions of native.supported with "the shapes of a dense block" replaced by "consistent
    pruned shapes", lost branches allowed.  (A dense tower satisfies them too; Transformer.forward asks native first.)"""
    if not len(transformer.resblocks):
        return False
    if not ((attn_mask is None or causal) and x.dim() == 3 and native._environment_ok(x) and transformer.head_dim == 64
            and x.shape[1] <= 2048 and x.dtype in (torch.float32, torch.bfloat16)):
        return False
    if not all(_block_supported(blk) for blk in transformer.resblocks):
        return False
    pl = plan(transformer, x.shape[-1])
    if pl is None or pl['Dp'] > MAX_STREAM:
        return False
    if torch.is_grad_enabled():
        # as native.supported: the backward writes a `.grad` for every parameter of every block
        flags = [p.requires_grad for p in transformer.resblocks.parameters()]
        if (x.requires_grad or any(flags)) and not all(flags):
            return False
    return True


class _Keep:
    """The hidden mask [1] * d + [0] * (Dp - d) as mask_ops' LayerNorm wrappers take it; n_keep from the shapes."""
    __slots__ = ("z", "n_keep")
    _cache = {}

    def __init__(self, z, n_keep):
        self.z, self.n_keep = z, n_keep

    @classmethod
    def of(cls, device, d, Dp):
        key = (device, d, Dp)
        hm = cls._cache.get(key)
        if hm is None:
            z = torch.zeros(Dp, dtype=torch.float32, device=device)
            z[:d] = 1.0
            hm = cls._cache[key] = cls(z, d)
        return hm


class PrunedOperands:
    """Padded operands of one pruned block, modelled on native.BlockOperands: per remaining branch the bf16 W (out, in) and
    W^T (in, out) copies and biases on the padded shapes — allocated ONCE as zeros; the copy launch writes the compact
    rows x cols and never touches the padding — and the padded fp32 gamma / beta of its LayerNorm.  Stale after any optimizer
    step (block._register's global post-step hook) or version change."""

    def __init__(self, blk, info, d, Dp):
        self.pairs, self.lns = [], []
        if info['attn']:
            at = blk.attn
            self.pairs += [(at.in_proj_weight, at.in_proj_bias, 3 * 64 * info['H'], Dp), (at.out_proj.weight, at.out_proj.bias, Dp, 64 * info['H'])]
            self.lns.append(blk.ln_1)
        if info['mlp']:
            mlp = blk.mlp
            self.pairs += [(mlp.c_fc.weight, mlp.c_fc.bias, info['Fp'], Dp), (mlp.c_proj.weight, mlp.c_proj.bias, Dp, info['Fp'])]
            self.lns.append(blk.ln_2)
        dev = self.pairs[0][0].device
        bf = dict(dtype=torch.bfloat16, device=dev)
        self.w = [torch.zeros((n, k), **bf) for _, _, n, k in self.pairs]
        self.wt = [torch.zeros((k, n), **bf) for _, _, n, k in self.pairs]
        self.b = [torch.zeros((n,), **bf) for _, _, n, _ in self.pairs]
        self.ln = [(torch.zeros(Dp, dtype=torch.float32, device=dev), torch.zeros(Dp, dtype=torch.float32, device=dev)) for _ in self.lns]
        self.shape = (d, Dp, info['attn'], info['mlp'], info['H'], info['F'])
        self.key = self._key()
        self.versions = None
        self._table = None
        K._register(self)

    def _params(self):
        return [p for w, b, _, _ in self.pairs for p in (w, b)] + [p for ln in self.lns for p in (ln.weight, ln.bias)]

    def _key(self):
        return tuple(p.data_ptr() for p in self._params())

    def _versions(self):
        return tuple(p._version for p in self._params())

    def refresh(self):
        if self._table is None:
            jobs = []
            for (w, b, _, _), mw, mwt, mb in zip(self.pairs, self.w, self.wt, self.b):
                jobs.append(K.param_job(w.detach(), mir=mw, mir_t=mwt))
                jobs.append(K.param_job(b.detach(), mir=mb))
            self._table = K.JobTable(jobs, self.w[0].device)
        self._table.launch(update=False)
        Dp = self.shape[1]
        for ln, (g, b) in zip(self.lns, self.ln):
            P.pad_cols(ln.weight.detach().view(1, -1), Dp, out=g.view(1, -1))
            P.pad_cols(ln.bias.detach().view(1, -1), Dp, out=b.view(1, -1))
        self.versions = self._versions()

    def stale(self):
        return self.versions != self._versions()

    def half(self, kind):
        """-> (w, wt, b lists of the branch's two projections, (gamma, beta) padded) of 'attn' | 'mlp'."""
        i = 0 if kind == 'attn' or not self.shape[2] else 1
        return self.w[2 * i:2 * i + 2], self.wt[2 * i:2 * i + 2], self.b[2 * i:2 * i + 2], self.ln[i]


def operands(blk, info, d, Dp):
    ops = blk.__dict__.get(_OPS_KEY)
    if ops is None or ops.shape != (d, Dp, info['attn'], info['mlp'], info['H'], info['F']) or ops.key != ops._key():
        ops = blk.__dict__[_OPS_KEY] = PrunedOperands(blk, info, d, Dp)
    if ops.stale():
        ops.refresh()
    return ops


def _ln_in(x, pend, L, gb, eps, hm):
    """The half's entry: the pending residual add folded into the masked LayerNorm.  -> (xin, y, mean, rstd)"""
    if pend is None:
        return (x,) + MO.ln_fwd_masked(x, gb[0], gb[1], eps, hm)
    return MO.add_ln_fwd_masked(x, pend, None, L, gb[0], gb[1], eps, hm)


def _attn_forward(blk, info, ops, x, pend, B, L, keep, causal, hm):
    """x (M, Dp) fp32 stream (before the add of `pend`, the previous half's branch output).  -> (xin, p, saved)"""
    M, Dp = x.shape
    H = info['H']
    inner = 64 * H
    (wqkv, wo), _, (bqkv, bo), gb = ops.half('attn')
    xin, a, mean, rstd = _ln_in(x, pend, L, gb, blk.ln_1.eps, hm)
    qkv = K.linear_fwd(a, wqkv, bqkv, 3 * inner, Dp)
    o, lse, _ = irpe_fused.fwd_core(qkv.view(B, L, 3, H, 64), 0.125, irpe_fused._NO_TERMS, 0.0, 0, causal)
    p = K.linear_fwd(o.view(M, inner), wo, bo, Dp, inner)
    return xin, p, ((xin, mean, rstd, a, qkv, o, lse) if keep else None)


def _mlp_forward(blk, info, ops, x, pend, B, L, keep, hm):
    """-> (xin, f, saved)"""
    M, Dp = x.shape
    Fp = info['Fp']
    (w1, w2), _, (b1, b2), gb = ops.half('mlp')
    xin, c, mean, rstd = _ln_in(x, pend, L, gb, blk.ln_2.eps, hm)
    gp, g = K.linear_gelu_fwd(c, w1, b1, Fp, Dp, want_grad=keep)
    f = K.linear_fwd(g, w2, b2, Dp, Fp)
    return xin, f, ((xin, mean, rstd, c, gp, g) if keep else None)


def _attn_backward(blk, info, ops, saved, dxo, dfo, pb, B, L, want_prev, causal, hm, d, jobs, held):
    """dxo (M, Dp) fp32 gradient of the stream behind the half's add, dfo (M, Dp) bf16 = the gradient of the branch output
    with its per-slab column sums pb = (tensor, nparts, pstride, offset).  -> (dx, df_prev, pb_prev)"""
    xin, mean, rstd, a, qkv, o, lse = saved
    M, Dp = xin.shape
    H = info['H']
    inner = 64 * H
    at, ln = blk.attn, blk.ln_1
    _, (wqkv_t, wo_t), _, gb = ops.half('attn')
    pwp, _ = K.wgrad_parts_async(dfo, o.view(M, inner))
    jobs.add(at.out_proj.weight, pwp, pwp.shape[0], Dp * inner, d, inner, inner)
    jobs.add(at.out_proj.bias, pb[0], pb[1], pb[2], 1, d, Dp, src_offset=pb[3])
    do = K.linear_dgrad(dfo, wo_t, Dp, inner)
    dqkv, _ = irpe_fused.bwd_core(do.view(B, L, inner), qkv.view(B, L, 3, H, 64), o, lse, None, 0.125, irpe_fused._NO_TERMS, 0.0, 0, causal)
    dqkv2d = dqkv.view(M, 3 * inner)
    pwq, pbq = K.wgrad_parts_async(dqkv2d, a, want_bias=True)
    jobs.add(at.in_proj_weight, pwq, pwq.shape[0], 3 * inner * Dp, 3 * inner, d, Dp)
    jobs.add(at.in_proj_bias, pbq, pbq.shape[0], 3 * inner, 1, 3 * inner, 3 * inner)
    da = K.linear_dgrad(dqkv2d, wqkv_t, 3 * inner, Dp)
    dx, df_prev, pl = MO.ln_bwd_masked_raw(da, xin, mean, rstd, gb[0], hm, dxo, None, L, want_prev)
    Pn = pl.shape[0]
    jobs.add(ln.weight, pl, Pn, 3 * Dp, 1, d, Dp)
    jobs.add(ln.bias, pl, Pn, 3 * Dp, 1, d, Dp, src_offset=Dp)
    held += [dfo, o, pwp, pb[0], dqkv, a, pwq, pbq, pl]
    return dx, df_prev, (pl, Pn, 3 * Dp, 2 * Dp)


def _mlp_backward(blk, info, ops, saved, dxo, dfo, pb, B, L, want_prev, hm, d, jobs, held):
    """As _attn_backward, for the MLP half."""
    xin, mean, rstd, c, gp, g = saved
    M, Dp = xin.shape
    F_, Fp = info['F'], info['Fp']
    mlp, ln = blk.mlp, blk.ln_2
    _, (w1_t, w2_t), _, gb = ops.half('mlp')
    pw2, _ = K.wgrad_parts_async(dfo, g)
    jobs.add(mlp.c_proj.weight, pw2, pw2.shape[0], Dp * Fp, d, F_, Fp)
    jobs.add(mlp.c_proj.bias, pb[0], pb[1], pb[2], 1, d, Dp, src_offset=pb[3])
    dh, pb1 = K.linear_dgrad_mul(dfo, w2_t, gp, Dp, Fp)
    pw1, _ = K.wgrad_parts_async(dh, c)
    jobs.add(mlp.c_fc.weight, pw1, pw1.shape[0], Fp * Dp, F_, d, Dp)
    jobs.add(mlp.c_fc.bias, pb1, pb1.shape[0], Fp, 1, F_, Fp)
    dc = K.linear_dgrad(dh, w1_t, Fp, Dp)
    dx, df_prev, pl = MO.ln_bwd_masked_raw(dc, xin, mean, rstd, gb[0], hm, dxo, None, L, want_prev)
    Pn = pl.shape[0]
    jobs.add(ln.weight, pl, Pn, 3 * Dp, 1, d, Dp)
    jobs.add(ln.bias, pl, Pn, 3 * Dp, 1, d, Dp, src_offset=Dp)
    held += [dfo, g, pw2, pb[0], dh, c, pw1, pb1, pl]
    return dx, df_prev, (pl, Pn, 3 * Dp, 2 * Dp)


def _halves(pl):
    """[(block index, 'attn' | 'mlp')] in forward order."""
    return [(i, kind) for i, info in enumerate(pl['blocks']) for kind in ('attn', 'mlp') if info[kind]]


class PrunedTowerStack(torch.autograd.Function):
    """x (B, L, d) fp32 | bf16 -> (B, L, d) same dtype: all remaining halves of a pruned tower."""

    @staticmethod
    def forward(ctx, x, blks, pl, causal, grad_mode, *params):
        B, L, d = x.shape
        M, Dp = B * L, pl['Dp']
        blks = list(blks)
        halves = _halves(pl)
        # needs_input_grad repeats the inputs' requires_grad whatever the grad mode, and inside forward the mode is always off:
        # the caller's mode comes as an argument, so that a forward under no_grad saves nothing and writes no gelu'
        keep = grad_mode and any(ctx.needs_input_grad)
        hm = _Keep.of(x.device, d, Dp)
        cur = P.pad_cols(x.reshape(M, d).contiguous(), Dp)
        pend = None
        saved, counts = [], []
        for i, kind in halves:
            blk, info = blks[i], pl['blocks'][i]
            ops = operands(blk, info, d, Dp)
            if kind == 'attn':
                cur, pend, sv = _attn_forward(blk, info, ops, cur, pend, B, L, keep, causal, hm)
            else:
                cur, pend, sv = _mlp_forward(blk, info, ops, cur, pend, B, L, keep, hm)
            if keep:
                saved.extend(sv)
                counts.append(len(sv))
        out = K.residual_add(cur, pend, None, L * Dp)
        ctx.blks, ctx.pl, ctx.halves, ctx.counts, ctx.dims = blks, pl, halves, counts, (B, L, d)
        ctx.in_dtype, ctx.causal, ctx.hm = x.dtype, causal, hm
        if keep:
            ctx.save_for_backward(*saved)
        return P.unpad_cols(out, d, x.dtype).view(B, L, d)

    @staticmethod
    def backward(ctx, dout):
        blks, pl, halves, (B, L, d), hm = ctx.blks, ctx.pl, ctx.halves, ctx.dims, ctx.hm
        tens = ctx.saved_tensors
        M, Dp = B * L, pl['Dp']
        ends = [0]
        for n in ctx.counts:
            ends.append(ends[-1] + n)
        dx = P.pad_cols(dout.reshape(M, d).contiguous(), Dp)
        df, part = K.scale_cast_colsum(dx, None, L)
        pb = (part, part.shape[0], Dp, 0)
        jobs, held = P.CompactGradJobs(), []
        for h in range(len(halves) - 1, -1, -1):
            i, kind = halves[h]
            blk, info = blks[i], pl['blocks'][i]
            ops = operands(blk, info, d, Dp)
            sv = tens[ends[h]:ends[h + 1]]
            if kind == 'attn':
                dx, df, pb = _attn_backward(blk, info, ops, sv, dx, df, pb, B, L, h > 0, ctx.causal, hm, d, jobs, held)
            else:
                dx, df, pb = _mlp_backward(blk, info, ops, sv, dx, df, pb, B, L, h > 0, hm, d, jobs, held)
            if h == 0 or halves[h - 1][0] != i:          # the block's first half: ONE finalisation launch for all its gradients
                K.finalize_on_side_stream(jobs, blk, held)
                jobs, held = P.CompactGradJobs(), []
        K.join_side_stream(dx.device)
        return (P.unpad_cols(dx, d, ctx.in_dtype).view(B, L, d),) + (None,) * (len(ctx.needs_input_grad) - 1)


def tower(transformer, x, causal=False):
    """Run the pruned `transformer.resblocks` natively.  The parameters are passed to the node only so that autograd
    schedules its backward (they receive their gradients in place, announced through block.on_grads_ready)."""
    pl = plan(transformer, x.shape[-1])
    if not _halves(pl):                             # every block lost both branches: the identity
        return x
    params = [p for p in transformer.parameters()]
    return PrunedTowerStack.apply(x, transformer.resblocks, pl, bool(causal), torch.is_grad_enabled(), *params)
