"""TinyCLIP towers under the learnable pruning masks on the framework's own kernels — the sibling of
cream_amd.tinyclip.native.TowerStack for `Transformer.forward(x, hidden_z=, heads_z=, intermediate_z=)`
(TinyCLIP/src/open_clip/model.py:285-315, :375-424 with the masks of l0module.py), one autograd node per tower under bf16
autocast.  The masks never touch an activation: with zh = hidden_z (D), zd = heads_z[l] (H, 64 columns per head),
zi = intermediate_z[l] (F) a masked block is the DENSE block of cream_amd.tinyclip.native on the effective operands

    Wo' = diag(zh) Wo diag(e(zd))    bo' = zh * bo         (out_proj)
    W2' = diag(zh) W2 diag(zi)       b2' = zh * b2         (c_proj)          in_proj and c_fc are untouched

— written as bf16 copies by ONE launch per block (cream_mask_pack; in_proj / c_fc keep the existing copy launch) — with
ln_1 / ln_2 as the masked LayerNorm (statistics over the kept columns, exact zeros elsewhere: cream_ln_fwd_masked /
cream_add_ln_fwd_masked / cream_ln_bwd_masked).  The fused attention kernels are unchanged, causal text tower included.

The backward is the dense backward on W'^T.  Its split-K weight-gradient partials are gradients of the EFFECTIVE weights;
cream_mask_grad_finalize turns them, at weight size and on the weight-gradient stream, into W.grad (+= r (x) c . G) and into the
masks' gradients: d zd[l], d zi[l] per block and four (D) rows per block for d zh, added once per tower in row order by the
library's own fixed-tree sum.  The masks enter the node as tensor inputs and their gradients leave as its returned gradients
(after the side stream is joined), so L0Module's log-alphas get theirs through ordinary autograd of the hard-concrete sample.
A mask that requires no gradient (eval, no_grad) costs nothing in the backward.

Not here: pruned towers (inner = 64 H_l != D: cream_amd.tinyclip.native_pruned, the dense node on zero-padded operands);
composed path: mha_z / ffn_z, QuickGELU towers, fp32, CPU.
"""
import torch

from .. import irpe_fused
from ..autoformer import block as K
from . import mask_ops as M
from . import native

_OPS_KEY = '_cream_tc_masked_operands'


class _Pairs:
    __slots__ = ("pairs",)

    def __init__(self, pairs):
        self.pairs = pairs


class MaskedOperands:
    """bf16 operands of one masked block: in_proj and c_fc as plain copies (native.BlockOperands: the existing copy launch),
    out_proj and c_proj as EFFECTIVE copies (cream_mask_pack).  The effective copies are new tensors whenever the masks or
    the weights changed — a training step draws new masks per forward, and the copies of an earlier forward may still be
    needed by its backward; in eval mode the deterministic masks keep their version and the pack is reused."""

    def __init__(self, view):
        self.view = view
        self.plain = native.BlockOperands(_Pairs([view.pairs[0], view.pairs[2]]))
        self.eff = None
        self.eff_key = None

    def effective(self, zh, zd, zi):
        (Wo, Bo), (W2, B2) = self.view.pairs[1], self.view.pairs[3]
        key = tuple((t.data_ptr(), t._version) for t in (zh, zd, zi, Wo, Bo, W2, B2))
        if self.eff is None or key != self.eff_key or self.plain.versions is None:
            bf = dict(dtype=torch.bfloat16, device=Wo.device)
            D, F_ = W2.shape
            wo, wo_t, bo = torch.empty((D, D), **bf), torch.empty((D, D), **bf), torch.empty((D,), **bf)
            w2, w2_t, b2 = torch.empty((D, F_), **bf), torch.empty((F_, D), **bf), torch.empty((D,), **bf)
            jobs = M.MaskPack()
            jobs.add(Wo.detach(), zh, zd, 64, mir=wo, mir_t=wo_t)
            jobs.add(Bo.detach(), None, zh, 1, mir=bo)
            jobs.add(W2.detach(), zh, zi, 1, mir=w2, mir_t=w2_t)
            jobs.add(B2.detach(), None, zh, 1, mir=b2)
            jobs.launch()
            self.eff, self.eff_key = (wo, wo_t, bo, w2, w2_t, b2), key
        if self.plain.stale():
            self.plain.refresh()
        return self.eff


def operands(blk, view):
    ops = blk.__dict__.get(_OPS_KEY)
    if ops is None or ops.plain.key != ops.plain._key():
        ops = blk.__dict__[_OPS_KEY] = MaskedOperands(view)
    return ops


def supported(transformer, x, attn_mask, causal, hidden_z, heads_z, intermediate_z):
    """The conditions of native.supported, and all three masks as fp32 device tensors of the shapes Transformer.forward has
    checked (heads_z (layers, H) or (H,), intermediate_z (layers, F) or (F,))."""
    for z in (hidden_z, heads_z, intermediate_z):
        if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.device == x.device):
            return False
    if not native.supported(transformer, x, attn_mask, causal):
        return False
    F_ = transformer.resblocks[0].mlp.c_fc.weight.shape[0]
    return (all(blk.mlp.c_fc.weight.shape[0] == F_ for blk in transformer.resblocks) and intermediate_z.shape[-1] == F_
            and heads_z.shape[-1] * 64 == transformer.width)


def _per_layer(z, n):
    return (z if z.dim() == 2 else z.unsqueeze(0).expand(n, -1)).contiguous()


def _block_forward(view, plain, eff, x, pend, B, L, keep, causal, hm):
    """native._block_forward on the effective operands, with the masked LayerNorm.  -> (x1, f, saved)"""
    Mr, D = x.shape
    H = view.heads
    F_ = view.pairs[2][0].shape[0]
    (wqkv, w1), (bqkv, b1) = plain.w, plain.b
    wo, _, bo, w2, _, b2 = eff
    ln1, ln2 = view.ln1, view.ln2
    if pend is None:
        xin = x
        a, mean1, rstd1 = M.ln_fwd_masked(x, ln1.weight, ln1.bias, ln1.eps, hm)
    else:
        xin, a, mean1, rstd1 = M.add_ln_fwd_masked(x, pend, None, L, ln1.weight, ln1.bias, ln1.eps, hm)
    qkv = K.linear_fwd(a, wqkv, bqkv, 3 * D, D)
    o, lse, sv = irpe_fused.fwd_core(qkv.view(B, L, 3, H, 64), view.scale, irpe_fused._NO_TERMS, 0.0, 0, causal)
    p = K.linear_fwd(o.view(Mr, D), wo, bo, D, D)
    x1, c, mean2, rstd2 = M.add_ln_fwd_masked(xin, p, None, L, ln2.weight, ln2.bias, ln2.eps, hm)
    gp, g = K.linear_gelu_fwd(c, w1, b1, F_, D, want_grad=keep)
    f = K.linear_fwd(g, w2, b2, D, F_)
    saved = (xin, mean1, rstd1, a, qkv, o, lse, x1, mean2, rstd2, c, gp, g, sv if sv is not None else lse) if keep else None
    return x1, f, saved


def _grad_of(p):
    """-> (p.grad, True when it was created here: the job then writes instead of adding to a zero fill)."""
    fresh = p.grad is None
    if fresh:
        p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
    return p.grad, fresh


def _sum_job(jobs, dst, src, nparts, pstride, cols, src_offset=0):
    """A cream_grad_finalize job into a plain buffer: dst (cols) = the sum of the parts."""
    j = jobs.jobs[jobs.n]
    j.dst, j.src = dst.data_ptr(), src.data_ptr() + src_offset * src.element_size()
    j.ld, j.pstride, j.nparts, j.rows, j.cols = cols, pstride, nparts, 1, cols
    j.interleave, j.src_bf16, j.overwrite = 0, 1 if src.dtype == torch.bfloat16 else 0, 1
    jobs.n += 1
    jobs.keep.append(src)


class _BlockFinalize:
    """What a block's backward leaves to the weight-gradient stream: the plain sums first (among them the two bias
    gradients of the effective operands), then the masked finalisation that reads them."""

    def __init__(self):
        self.plain, self.masked = K.GradJobs(), M.MaskGradJobs()

    def launch(self):
        self.plain.launch()
        self.masked.launch()


def _block_backward(blk, view, plain, eff, saved, dx2, df, pb2, B, L, want_prev, causal, hm, zh, zd, zi, mask_out):
    """native._block_backward on W'^T.  mask_out: None, or (rows (4, D) of the d zh sum, d zd[l] (H), d zi[l] (F))."""
    xin, mean1, rstd1, a, qkv, o, lse, x1, mean2, rstd2, c, gp, g, sv = saved
    Mr, D = xin.shape
    H = view.heads
    (Wqkv, Bqkv), (Wo, Bo), (W1, B1), (W2, B2) = view.pairs
    F_ = W1.shape[0]
    wqkv_t, w1_t = plain.wt
    _, wo_t, _, _, w2_t, _ = eff
    ln1, ln2 = view.ln1, view.ln2
    fin = _BlockFinalize()
    jobs, mj = fin.plain, fin.masked
    hrows, dzd, dzi = mask_out if mask_out is not None else ((None,) * 4, None, None)
    tmp = torch.empty((2, D), dtype=torch.float32, device=xin.device)         # d b2', d bo'
    pw2, _ = K.wgrad_parts_async(df, g)
    gW2, fresh = _grad_of(W2)
    mj.add(gW2, pw2, pw2.shape[0], D * F_, W2.detach(), zh, zi, 1, dr_out=hrows[0], dc_out=dzi, overwrite=fresh)
    _sum_job(jobs, tmp[0], pb2[0], pb2[1], pb2[2], D, src_offset=pb2[3])
    gB2, fresh = _grad_of(B2)
    mj.add(gB2, tmp[0], 1, D, B2.detach(), None, zh, 1, dc_out=hrows[1], overwrite=fresh)
    dh, pb1 = K.linear_dgrad_mul(df, w2_t, gp, D, F_)
    pw1, _ = K.wgrad_parts_async(dh, c)
    jobs.add(W1, pw1, pw1.shape[0], F_ * D, F_, D)
    jobs.add(B1, pb1, pb1.shape[0], F_, 1, F_)
    dc = K.linear_dgrad(dh, w1_t, F_, D)
    dx1, dp, pl2 = M.ln_bwd_masked_raw(dc, x1, mean2, rstd2, ln2.weight, hm, dx2, None, L, True)
    P = pl2.shape[0]
    jobs.add(ln2.weight, pl2, P, 3 * D, 1, D)
    jobs.add(ln2.bias, pl2, P, 3 * D, 1, D, src_offset=D)
    _sum_job(jobs, tmp[1], pl2, P, 3 * D, D, src_offset=2 * D)
    gBo, fresh = _grad_of(Bo)
    mj.add(gBo, tmp[1], 1, D, Bo.detach(), None, zh, 1, dc_out=hrows[3], overwrite=fresh)
    pwp, _ = K.wgrad_parts_async(dp, o.view(Mr, D))
    gWo, fresh = _grad_of(Wo)
    mj.add(gWo, pwp, pwp.shape[0], D * D, Wo.detach(), zh, zd, 64, dr_out=hrows[2], dc_out=dzd, overwrite=fresh)
    do = K.linear_dgrad(dp, wo_t, D, D)
    dqkv, _ = irpe_fused.bwd_core(do.view(B, L, D), qkv.view(B, L, 3, H, 64), o, lse, sv, view.scale, irpe_fused._NO_TERMS, 0.0, 0, causal)
    dqkv2d = dqkv.view(Mr, 3 * D)
    pwq, pbq = K.wgrad_parts_async(dqkv2d, a, want_bias=True)
    jobs.add(Wqkv, pwq, pwq.shape[0], 3 * D * D, 3 * D, D)
    jobs.add(Bqkv, pbq, pbq.shape[0], 3 * D, 1, 3 * D)
    da = K.linear_dgrad(dqkv2d, wqkv_t, 3 * D, D)
    dx, df_prev, pl1 = M.ln_bwd_masked_raw(da, xin, mean1, rstd1, ln1.weight, hm, dx1, None, L, want_prev)
    jobs.add(ln1.weight, pl1, P, 3 * D, 1, D)
    jobs.add(ln1.bias, pl1, P, 3 * D, 1, D, src_offset=D)
    held = [df, g, pw2, pb2[0], dh, c, pw1, pb1, pl2, dp, o, pwp, dqkv, a, pwq, pbq, pl1, tmp]
    held += [t for grp in mj.keep for t in grp if t is not None]
    K.finalize_on_side_stream(fin, blk, held)
    return dx, df_prev, (pl1, P, 3 * D, 2 * D)


class MaskedTowerStack(torch.autograd.Function):
    """x (B, L, D), hidden_z (D), heads_z (layers, H), intermediate_z (layers, F) -> (B, L, D) in x's dtype."""

    @staticmethod
    def forward(ctx, x, blks, causal, zh, zd, zi, *params):
        B, L, D = x.shape
        Mr = B * L
        blks = list(blks)
        views = [native.clip_view(blk) for blk in blks]
        keep = any(ctx.needs_input_grad)
        zh, zd, zi = zh.detach().contiguous(), zd.detach(), zi.detach()
        hm = M.HiddenMask(zh)
        cur = x.reshape(Mr, D).float().contiguous()
        pend = None
        saved, effs = [], []
        for i, (blk, view) in enumerate(zip(blks, views)):
            ops = operands(blk, view)
            eff = ops.effective(zh, zd[i], zi[i])
            x1, f, sv = _block_forward(view, ops.plain, eff, cur, pend, B, L, keep, causal, hm)
            if keep:
                saved.extend(sv)
                effs.append(eff)
            cur, pend = x1, f
        out = K.residual_add(cur, pend, None, L * D)
        ctx.blks, ctx.views, ctx.dims, ctx.nsaved = blks, views, (B, L, D), (len(saved) // len(blks) if keep else 0)
        ctx.in_dtype, ctx.causal, ctx.hm, ctx.effs, ctx.masks = x.dtype, causal, hm, effs, (zh, zd, zi)
        if keep:
            ctx.save_for_backward(*saved)
        return out.view(B, L, D).to(x.dtype)

    @staticmethod
    def backward(ctx, dout):
        blks, (B, L, D), ns = ctx.blks, ctx.dims, ctx.nsaved
        tens = ctx.saved_tensors
        zh, zd, zi = ctx.masks
        n = len(blks)
        want_masks = any(ctx.needs_input_grad[3:6])
        dev = dout.device
        if want_masks:
            hrows = torch.empty((4 * n, D), dtype=torch.float32, device=dev)
            dzd, dzi = torch.empty_like(zd), torch.empty_like(zi)
        dx = dout.reshape(B * L, D).float().contiguous()
        df, part = K.scale_cast_colsum(dx, None, L)
        pb2 = (part, part.shape[0], D, 0)
        for i in range(n - 1, -1, -1):
            blk, view = blks[i], ctx.views[i]
            mask_out = (tuple(hrows[4 * i + j] for j in range(4)), dzd[i], dzi[i]) if want_masks else None
            dx, df, pb2 = _block_backward(blk, view, operands(blk, view).plain, ctx.effs[i], tens[i * ns:(i + 1) * ns], dx, df, pb2, B, L,
                                          i > 0, ctx.causal, ctx.hm, zh, zd[i], zi[i], mask_out)
        dzh = None
        if want_masks:                                   # d zh = the 4 rows of every block, in row order, fixed tree; on the side stream
            dzh = torch.empty_like(zh)
            jobs = K.GradJobs()
            _sum_job(jobs, dzh, hrows, 4 * n, D, D)
            if K.WGRAD_SIDE_STREAM:
                side = K._side_stream(dev)
                side.wait_event(torch.cuda.current_stream(dev).record_event())
                with torch.cuda.stream(side):
                    jobs.launch()
            else:
                jobs.launch()
        K.join_side_stream(dev)
        need = ctx.needs_input_grad
        return ((dx.view(B, L, D).to(ctx.in_dtype), None, None, dzh if need[3] else None, dzd if need[4] and want_masks else None,
                 dzi if need[5] and want_masks else None) + (None,) * (len(need) - 6))


def tower(transformer, x, causal, hidden_z, heads_z, intermediate_z):
    """Run `transformer.resblocks` natively under the three masks (the parameters are passed so that autograd schedules the
    node's backward; they receive their gradients in place, like native.tower's)."""
    n = len(transformer.resblocks)
    params = [p for p in transformer.parameters()]
    return MaskedTowerStack.apply(x, transformer.resblocks, bool(causal), hidden_z, _per_layer(heads_z, n), _per_layer(intermediate_z, n),
                                  *params)
