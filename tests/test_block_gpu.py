"""GPU tests of the fused transformer block (cream_amd/autoformer/block.py on csrc/block_ops.hip):
each HBM-pass kernel against a plain PyTorch fp32 reference of the same op, and the whole block
(bf16 throughput mode) against the module path and the fp32 CPU oracle."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from fixture_utils import fill_params  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("M,E", [(197 * 3, 384), (1000, 216), (64, 448), (5, 1280)])
def test_layernorm_kernels_match_torch_fp32(M, E):
    from cream_amd.autoformer import block as K
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(M, E, device=DEV, generator=g) * 2 + 0.5
    w = torch.randn(E, device=DEV, generator=g)
    b = torch.randn(E, device=DEV, generator=g)
    dy = torch.randn(M, E, device=DEV, generator=g).bfloat16()
    dres = torch.randn(M, E, device=DEV, generator=g)
    xr = x.clone().requires_grad_()
    wr, br = w.clone().requires_grad_(), b.clone().requires_grad_()
    ref = F.layer_norm(xr, (E,), wr, br, 1e-5)
    ref.backward(dy.float())
    y, mean, rstd = K.ln_fwd(x, w, b, 1e-5)
    assert _rel(y.float(), ref) < 1e-2                                   # bf16 output rounding
    assert _rel(mean, x.mean(1)) < 1e-5 and _rel(rstd, (x.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
    rows = 7 if M % 7 == 0 else M
    scale = torch.rand(M // rows, device=DEV, generator=g) + 0.5
    dx, dxs, part = K.ln_bwd(dy, x, mean, rstd, w, dres, scale, rows, True)
    assert _rel(dx, xr.grad + dres) < 1e-5
    assert _rel(dxs.float(), (xr.grad + dres) * scale.repeat_interleave(rows)[:, None]) < 1e-2
    assert _rel(part[0], wr.grad) < 1e-4 and _rel(part[1], br.grad) < 1e-4
    assert _rel(part[2], dxs.float().sum(0)) < 1e-5                      # bias gradient rides along
    dx2, none, part2 = K.ln_bwd(dy, x, mean, rstd, w, None, None, 1, False)
    assert none is None and _rel(dx2, xr.grad) < 1e-5 and float(part2[2].abs().max()) == 0.0
    # residual add fused with the LayerNorm that follows it
    res = torch.randn(M, E, device=DEV, generator=g).bfloat16()
    x1, y1, mean1, rstd1 = K.add_ln_fwd(x, res, scale, rows, w, b, 1e-5)
    x1_ref = x + scale.repeat_interleave(rows)[:, None] * res.float()
    assert _rel(x1, x1_ref) < 1e-6
    assert _rel(y1.float(), F.layer_norm(x1_ref, (E,), w, b, 1e-5)) < 1e-2
    assert _rel(mean1, x1_ref.mean(1)) < 1e-5
    x1n, _, _, _ = K.add_ln_fwd(x, res, None, 1, w, b, 1e-5)
    assert _rel(x1n, x + res.float()) < 1e-6


def test_gelu_residual_scale_colsum_match_torch_fp32():
    from cream_amd.autoformer import block as K
    g = torch.Generator(device=DEV).manual_seed(1)
    M, C, rows = 197 * 4, 1344, 197
    h = (torch.randn(M, C, device=DEV, generator=g) * 2).bfloat16()
    dg = torch.randn(M, C, device=DEV, generator=g).bfloat16()
    hr = h.float().requires_grad_()
    ref = F.gelu(hr)
    ref.backward(dg.float())
    assert _rel(K.gelu_fwd(h).float(), ref) < 1e-2
    assert _rel(K.gelu_bwd(dg, h).float(), hr.grad) < 1e-2
    x = torch.randn(M, C, device=DEV, generator=g)
    s = torch.rand(M // rows, device=DEV, generator=g)
    srow = s.repeat_interleave(rows)[:, None]
    assert torch.equal(K.residual_add(x, h, s, rows * C), x + srow * h.float())
    assert torch.equal(K.residual_add(x, h, None, rows * C), x + h.float())
    assert _rel(K.scale_cast(x, s, rows * C).float(), x * srow) < 1e-2
    assert _rel(K.colsum(h), h.float().sum(0)) < 1e-5
    assert _rel(K.wgrad(dg, h), dg.float().t() @ h.float()) < 1e-3


@pytest.mark.parametrize("M,C", [(197 * 4, 1344), (130, 320), (25216, 448)])
def test_passes_with_bias_gradient_match_torch_fp32(M, C):
    """gelu_bwd / scale_cast with the column sums riding along, against the two-kernel form."""
    from cream_amd.autoformer import block as K
    g = torch.Generator(device=DEV).manual_seed(2)
    rows = 197 if M % 197 == 0 else M
    h = (torch.randn(M, C, device=DEV, generator=g) * 2).bfloat16()
    dg = torch.randn(M, C, device=DEV, generator=g).bfloat16()
    dh, part = K.gelu_bwd_colsum(dg, h)
    assert torch.equal(dh, K.gelu_bwd(dg, h))
    assert _rel(part.sum(0), dh.float().sum(0)) < 1e-5
    x = torch.randn(M, C, device=DEV, generator=g)
    s = torch.rand(M // rows, device=DEV, generator=g)
    out, part = K.scale_cast_colsum(x, s, rows)
    assert torch.equal(out, K.scale_cast(x, s, rows * C))
    assert _rel(part.sum(0), out.float().sum(0)) < 1e-5
    assert _rel(K.colsum128(h).sum(0), h.float().sum(0)) < 1e-5


@pytest.mark.parametrize("M,N,K,ldw", [(197 * 8, 1152, 384, 384), (197 * 8, 1344, 384, 448), (25216, 384, 1344, 1792),
                                        (197 * 8, 320, 320, 448), (25216, 1344, 448, 448), (1000, 200, 136, 144),
                                        (197 * 8, 320, 1120, 1792)])
def test_native_linear_matches_torch_fp32(M, N, K, ldw):
    """cream_linear_fwd / dgrad / wgrad_parts (hand-written MFMA kernels through the C ABI, active
    block of the super weight read in place) against plain PyTorch fp32 of the same products:
    every tile variant (N above / below 640), row / column edges, K tails (136, 1120 % 64 != 0)."""
    from cream_amd.autoformer import block as K_
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    wsup = (torch.randn(N + 64, ldw, device=DEV, generator=g) * 0.05).bfloat16()
    bias = torch.randn(N + 64, device=DEV, generator=g).bfloat16()
    dy = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    W = wsup[:N, :K].float()
    wt = torch.zeros(ldw, N + 64, device=DEV, dtype=torch.bfloat16)          # transposed operand copy (in, out)
    wt[:, :] = wsup.t()
    out = K_.linear_fwd(x, wsup, bias, N, K)
    assert _rel(out.float(), x.float() @ W.t() + bias[:N].float()) < 1e-2
    assert _rel(K_.linear_fwd(x, wsup, None, N, K).float(), x.float() @ W.t()) < 1e-2
    dx = K_.linear_dgrad(dy, wt, N, K)
    assert _rel(dx.float(), dy.float() @ W) < 1e-2
    parts, bparts = K_.linear_wgrad_parts(dy, x, want_bias=True)
    assert parts.shape[1:] == (N, K) and parts.dtype == torch.float32
    assert _rel(parts.sum(0), dy.float().t() @ x.float()) < 1e-3           # fp32 partials: only bf16 operand rounding left
    assert _rel(bparts.sum(0), dy.float().sum(0)) < 1e-4
    assert torch.equal(K_.linear_wgrad_parts(dy, x)[0], parts)             # bit-reproducible, bias output optional
    # nothing outside the active block was touched or read: a poisoned remainder changes nothing
    wsup2 = wsup.clone()
    wsup2[N:] = float("nan")
    wsup2[:, K:] = float("nan")
    wt2 = wt.clone()
    wt2[K:] = float("nan")
    wt2[:, N:] = float("nan")
    assert torch.equal(K_.linear_fwd(x, wsup2, bias, N, K), out)
    assert torch.equal(K_.linear_dgrad(dy, wt2, N, K), dx)
    # outputs are exactly M x N: a guard band after the buffer stays untouched
    buf = torch.full((M * N + 4096,), -7.0, device=DEV).bfloat16()
    K_.linear_fwd(x, wsup, bias, N, K, out=buf[:M * N].view(M, N))
    assert torch.equal(buf[:M * N].view(M, N), out) and bool((buf[M * N:] == -7).all())


@pytest.mark.parametrize("M,E,H", [(197 * 8, 384, 6), (25216, 320, 5), (197 * 4, 448, 7)])
def test_qkv_segment_addressing_matches_row_gather(M, E, H):
    """The de-interleaved [q | k | v] operand copies (written by the optimizer kernel) reproduce the
    row gather of qkv_super.py:72-77 in forward and dgrad; contiguous-prefix bias (:80-83)."""
    from cream_amd.autoformer import block as K_, engine
    torch.manual_seed(0)
    blk = engine.build_supernet("S", depth=1).to(DEV).blocks[0]
    with torch.no_grad():
        blk.attn.qkv.bias.normal_()
    Q = 64 * H
    ops = K_.operands(blk)
    Wsup, bsup = blk.attn.qkv.weight.detach(), blk.attn.qkv.bias.detach()
    Wg = torch.cat([Wsup[i:3 * Q:3, :E] for i in range(3)], dim=0).bfloat16().float()      # the reference's gather
    assert torch.equal(ops.w[0][:, :Q, :E].reshape(3 * Q, E).float(), Wg)
    assert torch.equal(ops.wt[0][:, :E, :Q].float(), ops.w[0][:, :Q, :E].transpose(1, 2).float())
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(M, E, device=DEV, generator=g).bfloat16()
    dy = torch.randn(M, 3 * Q, device=DEV, generator=g).bfloat16()
    out = K_.linear_fwd_seg(x, ops.w[0], ops.b[0], 3 * Q, E, Q)
    assert _rel(out.float(), x.float() @ Wg.t() + bsup[:3 * Q].bfloat16().float()) < 1e-2
    dx = K_.linear_dgrad_seg(dy, ops.wt[0], 3 * Q, E, Q)
    assert _rel(dx.float(), dy.float() @ Wg) < 1e-2


@pytest.mark.parametrize("M,E,F_", [(197 * 8, 384, 1344), (25216, 448, 1792), (1000, 320, 1120), (197 * 4, 320, 960)])
def test_fused_gelu_epilogues_match_unfused_passes(M, E, F_):
    """fc1 with the erf-GELU in its epilogue: g == gelu(float(h)) and gp == gelu'(float(h)) for the
    bf16-rounded h = fc1(c) (what the reference computes under autocast) within one bf16 ulp (the epilogue
    evaluates erf by A&S 7.1.26, |err| <= 5e-7); fc2's dgrad with the saved derivative in its epilogue ==
    (fp32 accumulator, not bf16-rounded first) * gelu'(h), and the column-sum partials add up to the
    column sums of what was written."""
    from cream_amd.autoformer import block as K_
    g = torch.Generator(device=DEV).manual_seed(5)
    c = torch.randn(M, E, device=DEV, generator=g).bfloat16()
    w1 = (torch.randn(F_, E, device=DEV, generator=g) * 0.08).bfloat16()
    b1 = torch.randn(F_, device=DEV, generator=g).bfloat16()
    gp, gg = K_.linear_gelu_fwd(c, w1, b1, F_, E)
    h = K_.linear_fwd(c, w1, b1, F_, E)                      # the bf16 h the epilogue worked on
    hr = h.float().requires_grad_()
    ref_g = F.gelu(hr)
    ref_g.sum().backward()
    ref_gp = hr.grad
    assert _rel(gg.float(), ref_g) < 4e-3 and float((gg.float() - ref_g).abs().max()) <= 2 ** -7 * float(ref_g.abs().max())
    assert _rel(gg.float(), K_.gelu_fwd(h).float()) < 4e-3
    assert _rel(gp.float(), ref_gp) < 4e-3
    df = torch.randn(M, E, device=DEV, generator=g).bfloat16()
    w2 = (torch.randn(E, F_, device=DEV, generator=g) * 0.05).bfloat16()
    w2t = w2.t().contiguous()
    dh, parts = K_.linear_dgrad_mul(df, w2t, gp, E, F_)
    assert _rel(dh.float(), (df.float() @ w2.float()) * ref_gp) < 1e-2
    assert parts.shape == (K_._lib.load().cream_colsum128_slabs(M), F_)
    assert _rel(parts.sum(0), dh.float().sum(0)) < 1e-5


def test_native_adamw_matches_torch_and_writes_operand_copies():
    """cream_adamw_step (one launch over all tensors) against torch.optim.AdamW on the same gradients
    for several steps (both parameter groups), and the bf16 operand copies it writes: W, W^T, the
    de-interleaved qkv parts, biases."""
    from cream_amd.autoformer import block as K_, engine
    torch.manual_seed(3)
    m = engine.build_supernet("S", depth=2).to(DEV)
    ref = engine.build_supernet("S", depth=2).to(DEV)
    ref.load_state_dict(m.state_dict())
    opt = engine.build_optimizer(m, lr=2e-2, batch_size=128)
    assert isinstance(opt, engine.NativeAdamW)
    opt_ref = torch.optim.AdamW(engine.param_groups(ref, 0.05), lr=2e-2 * 128 / 512, betas=(0.9, 0.999), eps=1e-8)
    g = torch.Generator(device=DEV).manual_seed(7)
    for step in range(3):
        for p, q in zip(m.parameters(), ref.parameters()):
            gr = torch.randn(p.shape, device=DEV, generator=g) * 0.1
            if p.grad is None:
                p.grad = gr.clone()
            else:
                p.grad.copy_(gr)
            q.grad = gr.clone()
        opt.step()
        opt_ref.step()
    worst = 0.0
    for (n, p), q in zip(m.named_parameters(), ref.parameters()):
        worst = max(worst, float((p - q).abs().max() / (q.abs().max() + 1e-12)))
    assert worst < 2e-6, worst
    st, st_ref = opt.state[m.blocks[1].fc1.weight], opt_ref.state[ref.blocks[1].fc1.weight]
    assert _rel(st["exp_avg"], st_ref["exp_avg"]) < 1e-6 and _rel(st["exp_avg_sq"], st_ref["exp_avg_sq"]) < 1e-6
    for blk in m.blocks:
        ops = K_.operands(blk, fresh=False)
        assert not ops.stale()
        for mod, w, wt, b in zip(ops.mods, ops.w, ops.wt, ops.b):
            W = mod.weight.detach().bfloat16()
            if w.dim() == 3:
                W = torch.stack([W[i::3] for i in range(3)])
            assert torch.equal(w, W) and torch.equal(wt, W.transpose(-1, -2))
            assert torch.equal(b, mod.bias.detach().bfloat16())
    # state dict round trip through torch's format
    sd = opt.state_dict()
    opt2 = engine.build_optimizer(m, lr=2e-2, batch_size=128)
    opt2.load_state_dict(sd)
    assert opt2._steps == 3 and torch.equal(opt2.state[m.blocks[1].fc1.weight]["exp_avg"], st["exp_avg"])


def test_grad_finalize_adds_partials_into_super_weight_slices():
    """cream_grad_finalize: many tensors in one launch, strided destination slices, the qkv row
    interleave (qkv_super.py:75), bf16 and fp32 partials, accumulation (+=), reproducible bits."""
    from cream_amd.autoformer import block as K
    g = torch.Generator(device=DEV).manual_seed(3)
    Q, E, SE = 128, 216, 256
    w = torch.nn.Parameter(torch.zeros(448, SE, device=DEV))            # plain slice W[:out, :in]
    wq = torch.nn.Parameter(torch.zeros(3 * 192, SE, device=DEV))       # interleaved qkv rows
    bias = torch.nn.Parameter(torch.zeros(448, device=DEV))
    tab = torch.nn.Parameter(torch.zeros(30, 64, device=DEV))
    w.grad = torch.randn(448, SE, device=DEV, generator=g)
    wq.grad = torch.randn(3 * 192, SE, device=DEV, generator=g)
    bias.grad = torch.randn(448, device=DEV, generator=g)
    before = [p.grad.clone() for p in (w, wq, bias, tab) if p.grad is not None]
    pw = torch.randn(8, 320, E, device=DEV, generator=g).bfloat16()
    pq = torch.randn(8, 3 * Q, E, device=DEV, generator=g).bfloat16()
    pb = torch.randn(197, 320, device=DEV, generator=g)
    pt = torch.randn(768, 4, 32, 64, device=DEV, generator=g)

    def run():
        jobs = K.GradJobs()
        jobs.add(w, pw, 8, 320 * E, 320, E)
        jobs.add(wq, pq, 8, 3 * Q * E, 3 * Q, E, interleave=Q)
        jobs.add(bias, pb, 197, 320, 1, 320)
        jobs.add(tab, pt, 768, 4 * 32 * 64, 30, 64, src_offset=2 * 32 * 64)
        jobs.launch()

    run()
    ref_w = before[0].clone()
    ref_w[:320, :E] += pw.float().sum(0)
    assert _rel(w.grad, ref_w) < 1e-6 and torch.equal(w.grad[320:], before[0][320:]) \
        and torch.equal(w.grad[:, E:], before[0][:, E:])
    ref_q = before[1].clone()
    ref_q[:3 * Q].view(Q, 3, SE)[:, :, :E] += pq.float().sum(0).view(3, Q, E).transpose(0, 1)
    assert _rel(wq.grad, ref_q) < 1e-6
    ref_b = before[2].clone()
    ref_b[:320] += pb.sum(0)
    assert _rel(bias.grad, ref_b) < 1e-5
    assert _rel(tab.grad, pt[:, 2, :30].sum(0)) < 1e-5                  # grad was None: created as zeros
    first = [p.grad.clone() for p in (w, wq, bias, tab)]
    for p, b0 in zip((w, wq, bias), before):
        p.grad.copy_(b0)
    tab.grad.zero_()
    run()
    assert all(torch.equal(a, p.grad) for a, p in zip(first, (w, wq, bias, tab)))   # fixed summation tree
    # overwrite mode (cream_grad_job.overwrite: a gradient that did not exist yet is allocated uninitialised and WRITTEN): whatever
    # the destination held must not come through — bf16 (8-wide chunks) and fp32 (4-wide) partials
    for parts, rows, cols in ((torch.randn(12, 64, 96, device=DEV, generator=g).bfloat16(), 64, 96), (torch.randn(200, 1, 76, device=DEV, generator=g), 1, 76)):
        p = torch.nn.Parameter(torch.zeros(rows, cols, device=DEV).squeeze(0))
        p.grad = torch.full_like(p, float("nan"))
        jobs = K.GradJobs()
        jobs.add(p, parts, parts.shape[0], rows * cols, rows, cols)
        assert jobs.jobs[0].overwrite == 0                       # an existing gradient is accumulated into
        jobs.jobs[0].overwrite = 1
        jobs.launch()
        assert torch.isfinite(p.grad).all() and _rel(p.grad, parts.float().sum(0).view_as(p)) < 1e-6
        q = torch.nn.Parameter(torch.zeros_like(p))
        jobs = K.GradJobs()
        jobs.add(q, parts, parts.shape[0], rows * cols, rows, cols)
        assert jobs.jobs[0].overwrite == 1                       # no gradient yet + the job covers the parameter
        jobs.launch()
        assert torch.equal(q.grad, p.grad)


def _supernet(depth=2):
    from cream_amd.autoformer import engine
    m = engine.build_supernet("S", drop_path_rate=0.0, depth=depth)
    fill_params(m, seed=7)
    return m


def test_fused_block_matches_module_path_and_oracle():
    """bf16 throughput mode: the fused block must be as close to the fp32 CPU oracle as PyTorch's
    own bf16 autocast of the module path is (documented tolerance 3e-2 on gradients)."""
    from cream_amd.autoformer import engine
    from oracle import autoformer_oracle as AO
    m = _supernet()
    cfg = dict(layer_num=2, embed_dim=[384, 384], num_heads=[6, 5], mlp_ratio=[3.5, 3.0])
    g = torch.Generator().manual_seed(5)
    images = torch.randn(2, 3, 224, 224, generator=g)
    target = torch.softmax(torch.randn(2, 1000, generator=g), -1)
    loss_ref, grads_ref = AO.train_step({k: v.detach().clone() for k, v in m.named_parameters()}, cfg, images, target)
    m = m.to(DEV)
    m.set_sample_config(cfg)
    m.train()
    res = {}
    for fused in (False, True):
        for blk in m.blocks:
            blk.fused = fused
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = engine.soft_target_cross_entropy(m(images.to(DEV)), target.to(DEV))
        loss.backward()
        res[fused] = (float(loss), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert set(res[True][1]) == set(res[False][1])
    assert abs(res[True][0] - float(loss_ref)) / float(loss_ref) < 5e-3
    worst_fused = max(_rel(v, grads_ref[k]) for k, v in res[True][1].items())
    worst_module = max(_rel(v, grads_ref[k]) for k, v in res[False][1].items())
    assert worst_fused < 3e-2, (worst_fused, worst_module)
    # structure: nothing outside the sampled slices
    gq = res[True][1]["blocks.1.attn.qkv.weight"]
    assert torch.count_nonzero(gq[:, 384:]) == 0 and torch.count_nonzero(gq[3 * 320:, :]) == 0
    assert torch.count_nonzero(res[True][1]["blocks.0.fc1.weight"][int(384 * 3.5):]) == 0


def test_frozen_parameters_keep_the_composed_path_and_get_no_gradient():
    """The native nodes write every parameter gradient of the node: with a frozen parameter inside a block (or in the
    stem / classifier) that node must fall back to the module path, `.grad` of the frozen tensor stays None and the
    other gradients agree with the all-trainable run."""
    from cream_amd.autoformer import engine
    m = _supernet().to(DEV)
    cfg = dict(layer_num=2, embed_dim=[384, 384], num_heads=[6, 6], mlp_ratio=[3.5, 3.5])
    m.set_sample_config(cfg)
    m.train()
    g = torch.Generator().manual_seed(9)
    images = torch.randn(2, 3, 224, 224, generator=g).to(DEV)
    target = torch.softmax(torch.randn(2, 1000, generator=g), -1).to(DEV)

    def run():
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = engine.soft_target_cross_entropy(m(images), target)
        loss.backward()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    full = run()
    frozen = ["blocks.1.fc1.weight", "head.bias", "cls_token"]
    params = dict(m.named_parameters())
    for k in frozen:
        params[k].requires_grad_(False)
    part = run()
    for k in frozen:
        assert params[k].grad is None and k not in part
    assert set(part) == set(full) - set(frozen)
    worst = max(_rel(part[k], full[k]) for k in part)
    assert worst < 3e-2, worst


def test_block_stack_equals_block_by_block_with_drop_path():
    """The run of blocks as one node (boundary passes merged: residual add on the next LayerNorm,
    fc2-output gradient out of the next LayerNorm's backward) against the same blocks applied one
    by one with the same drop-path scales: same arithmetic per element, so bit-identical output
    and input gradient, parameter gradients to summation-order noise."""
    from cream_amd.autoformer import block as K
    m = _supernet(depth=3).to(DEV)
    cfg = dict(layer_num=3, embed_dim=[384] * 3, num_heads=[6, 5, 7], mlp_ratio=[3.5, 3.0, 4.0])
    m.set_sample_config(cfg)
    m.train()
    g = torch.Generator(device=DEV).manual_seed(11)
    B = 4
    x0 = torch.randn(B, 197, 384, device=DEV, generator=g)
    scales = (torch.rand(3, 2, B, device=DEV, generator=g) > 0.3).float() / 0.7
    dout = torch.randn(B, 197, 384, device=DEV, generator=g)
    blks = list(m.blocks)
    res = []
    for stacked in (True, False):
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_()
        if stacked:
            y = K.StackFunction.apply(x, scales, blks)
        else:
            y = x
            for i, blk in enumerate(blks):
                y = K.BlockFunction.apply(y, scales[i, 0], scales[i, 1], blk)
        y.backward(dout)
        res.append((y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()
                                                         if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    assert set(res[0][2]) == set(res[1][2]) and len(res[0][2]) >= 3 * 16
    for k, v in res[0][2].items():
        assert _rel(v, res[1][2][k]) < 1e-5, k


def test_native_block_sequencing_equals_op_by_op_driving():
    """cream_block_fwd / cream_block_bwd (one C call per block and direction, weight gradients and
    finalisation on the side stream) against the same kernels driven op by op from Python on one
    stream: identical kernels on identical inputs in the same summation order -> identical bits."""
    from cream_amd.autoformer import block as K
    m = _supernet(depth=3).to(DEV)
    cfg = dict(layer_num=3, embed_dim=[448] * 3, num_heads=[7, 5, 6], mlp_ratio=[4.0, 3.0, 3.5])
    m.set_sample_config(cfg)
    m.train()
    g = torch.Generator(device=DEV).manual_seed(12)
    B = 4
    x0 = torch.randn(B, 197, 448, device=DEV, generator=g)
    scales = (torch.rand(3, 2, B, device=DEV, generator=g) > 0.3).float() / 0.7
    dout = torch.randn(B, 197, 448, device=DEV, generator=g)
    blks = list(m.blocks)
    res = []
    try:
        for native, side, sc in ((True, True, scales), (False, False, scales), (True, False, None), (False, True, None)):
            K.NATIVE_BLOCK, K.WGRAD_SIDE_STREAM = native, side
            m.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_()
            y = K.StackFunction.apply(x, sc, blks)
            y.backward(dout)
            torch.cuda.synchronize()
            res.append((y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()
                                                             if p.grad is not None}))
    finally:
        K.NATIVE_BLOCK, K.WGRAD_SIDE_STREAM = True, True
    for a, b in ((0, 1), (2, 3)):
        assert torch.equal(res[a][0], res[b][0]) and torch.equal(res[a][1], res[b][1])
        assert set(res[a][2]) == set(res[b][2]) and len(res[a][2]) >= 3 * 16
        for k, v in res[a][2].items():
            assert torch.equal(v, res[b][2][k]), k


def test_mirror_follows_optimizer_and_droppath_runs():
    from cream_amd.autoformer import block as K, engine
    m2 = engine.build_supernet("S", drop_path_rate=0.5, depth=2).to(DEV)
    opt = engine.build_optimizer(m2, batch_size=4)
    tr = engine.SupernetTrainer(m2, opt, engine.SEARCH_SPACES["S"]["choices"])
    x = torch.randn(4, 3, 224, 224, device=DEV)
    t = torch.softmax(torch.randn(4, 1000, device=DEV), -1)
    tr.start_epoch(0)
    l0 = float(tr.step(x, t))
    w = m2.blocks[0].fc1.weight
    ops = K.operands(m2.blocks[0], fresh=False)
    assert not ops.stale() and torch.equal(ops.w[2], w.detach().bfloat16())   # rewritten by the optimizer kernel
    assert torch.equal(ops.wt[2], w.detach().bfloat16().t())
    l1 = float(tr.step(x, t))
    assert l0 == l0 and l1 == l1


def test_reducer_bucket_protocol_with_fused_blocks(monkeypatch):
    """One process cannot run RCCL with itself, so the collective is stubbed: every active bucket
    must be all-reduced exactly once per step, after its last gradient was written (fused blocks
    announce theirs explicitly), blocks beyond the sampled depth are never sent, and the result
    is the SUM scaled by 1/world."""
    import torch.distributed as dist
    from cream_amd import comm
    from cream_amd.autoformer import engine
    calls = []

    def fake_all_reduce(t, op=None, group=None, async_op=False):
        calls.append((t.data_ptr(), t.numel(), float(t.abs().sum())))
        t.mul_(2.0)                                   # "sum over 2 identical ranks"
    monkeypatch.setattr(dist, "all_reduce", fake_all_reduce)
    torch.manual_seed(0)
    m = engine.build_supernet("S", drop_path_rate=0.0, depth=3).to(DEV)
    red = comm.GradReducer(m, world=2)
    try:
        opt = engine.build_optimizer(m, batch_size=2)
        tr = engine.SupernetTrainer(m, opt, engine.SEARCH_SPACES["S"]["choices"], red)
        tr.config = dict(layer_num=2, embed_dim=[320] * 2, num_heads=[5, 6], mlp_ratio=[3.0, 4.0])
        m.set_sample_config(tr.config)
        m.train()
        x = torch.randn(2, 3, 224, 224, device=DEV)
        t = torch.softmax(torch.randn(2, 1000, device=DEV), -1)
        # reference gradients without the reducer's scaling: single-process autograd on a copy
        tr.forward_backward(x, t)
        torch.cuda.synchronize()
        ptrs = {red.flat[b].data_ptr(): b for b in red.flat}
        ptrs.update({plan[0].data_ptr(): b for b, plan in red.msg.items()})    # active-slice messages (staging arena)
        assert set(red.msg) == {"block00", "block01", "stem", "tail"}
        sent = [ptrs[c[0]] for c in calls]
        # a message holds exactly the elements this configuration can write (E = 320, H = 5 / 6, ratio 3 / 4)
        assert sum(c[1] for c in calls) * 4 == red.bytes_sent < sum(red.flat[b].numel() for b in red.active) * 4
        assert sorted(sent) == ["block00", "block01", "stem", "tail"]          # block02 is beyond the depth
        assert all(c[2] > 0 for c in calls), "a bucket was sent before its gradients were written"
        # reverse layer order, stem last: communication overlaps the rest of backward
        assert sent[-1] == "stem" and sent.index("block01") < sent.index("block00")
        assert float(red.flat["block02"].abs().sum()) == 0.0
        g1 = m.blocks[0].fc1.weight.grad.clone()
        calls.clear()
        for blk in m.blocks:
            blk.fused = False                                                 # module path: autograd hooks
        tr.forward_backward(x, t)
        torch.cuda.synchronize()
        ptrs.update({plan[0].data_ptr(): b for b, plan in red.msg.items()})
        assert sorted(ptrs[c[0]] for c in calls) == ["block00", "block01", "stem", "tail"]
        assert _rel(m.blocks[0].fc1.weight.grad, g1) < 3e-2                   # (2x sum) / 2 either way
    finally:
        red.close()


# measured on the MI355X (round 2, gpurun_out r02i) over E/H = 320/5, 384/6, 448/7: worst max-abs error /
# max-abs reference of a B = 128 block in the bf16 throughput mode: y, dx < 4e-3; projection weight
# gradients <= 6.8e-3 (qkv); LayerNorm parameters <= 7.0e-3; position tables <= 8.2e-3.  Bounds = 2x.
B128_TOL = dict(y=8e-3, dx=8e-3, weights=1.4e-2, small=1.7e-2)


@pytest.mark.parametrize("E,H,R", [(320, 5, 3.0), (384, 6, 3.5), (448, 7, 4.0)])
def test_block_at_bench_batch_matches_oracle(E, H, R):
    """The benchmarked configuration itself: ONE supernet-S block at B = 128 (M = 25,216 rows: the
    768..896-workgroup attention grids, split-K weight gradients over all tokens, 197 column-sum
    slabs, 1024-slab LayerNorm partials) through the native bf16 path against the fp32 CPU oracle
    (oracle/autoformer_oracle.py: the reference's dense formulation) — forward output, input gradient
    and every parameter gradient."""
    from cream_amd.autoformer import block as K, engine
    from oracle import autoformer_oracle as AO
    torch.manual_seed(0)
    m = engine.build_supernet("S", drop_path_rate=0.0, depth=1)
    fill_params(m, seed=21)
    blk = m.blocks[0]
    cfg = dict(layer_num=1, embed_dim=[E], num_heads=[H], mlp_ratio=[R])
    m.set_sample_config(cfg)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(128, 197, E, generator=g)
    dy = torch.randn(128, 197, E, generator=g) / E ** 0.5
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.named_parameters() if k.startswith("blocks.0.")}
    xr = x.clone().requires_grad_(True)
    yr = AO.block(sd, 0, xr, E, H, R)
    yr.backward(dy)
    m = m.to(DEV)
    m.train()
    xd = x.to(DEV).requires_grad_(True)
    assert K.supported(blk, xd)
    y = K.StackFunction.apply(xd, None, [blk])
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    errs = {"y": _rel(y, yr), "dx": _rel(xd.grad, xr.grad)}
    for name, p in blk.named_parameters():
        ref = sd["blocks.0." + name].grad
        assert ref is not None and p.grad is not None, name
        errs[name] = _rel(p.grad, ref)
    print(f"[B=128 block E={E} H={H}] " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(errs.items(), key=lambda t: -t[1])[:8]))
    assert errs["y"] < B128_TOL["y"] and errs["dx"] < B128_TOL["dx"], errs
    for name in errs:
        if name in ("y", "dx"):
            continue
        tol = B128_TOL["weights"] if name.endswith("weight") and "norm" not in name else B128_TOL["small"]
        assert errs[name] < tol, (name, errs[name])


def test_patch_embedding_on_own_gemms_matches_fp32():
    """PatchembedSuper under bf16 autocast runs the NT / TN GEMMs of csrc/gemm_mfma.hpp (embedding_super.py:27-40
    is a stride = kernel convolution = a GEMM over unfolded patches): output, weight and bias gradient against the
    fp32 module; rows beyond the sampled width receive exactly zero gradient."""
    from cream_amd import timing
    from cream_amd.autoformer.modules import PatchembedSuper
    torch.manual_seed(5)
    pe = PatchembedSuper(img_size=224, patch_size=16, in_chans=3, embed_dim=448).to(DEV)
    pe.set_sample_config(384)
    x = torch.randn(16, 3, 224, 224, device=DEV)
    gy = torch.randn(16, 196, 384, device=DEV)
    ref = pe(x)
    gw_ref, gb_ref = torch.autograd.grad(ref, [pe.proj.weight, pe.proj.bias], gy)
    timing.reset()
    timing.enable(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = pe(x)
    gw, gb = torch.autograd.grad(y, [pe.proj.weight, pe.proj.bias], gy.to(y.dtype))
    timing.enable(False)
    assert {"gemm_nt", "gemm_tn_wgrad"} <= set(timing.summary()), "the native GEMMs did not run"
    rel = lambda a, b: float((a.float() - b).abs().max() / b.abs().max())      # noqa: E731
    errs = dict(y=rel(y, ref), gw=rel(gw, gw_ref), gb=rel(gb, gb_ref))
    print("[patch embed]", errs)
    assert y.dtype == torch.bfloat16 and errs["y"] < 1e-2 and errs["gw"] < 1e-2 and errs["gb"] < 1e-2
    assert float(gw[384:].abs().max()) == 0.0 and float(gb[384:].abs().max()) == 0.0


def test_native_stem_and_tail_match_the_module_path():
    """forward_features' two ends on csrc/stem_tail.hip (unfold + GEMM + class token + position embedding; final
    LayerNorm + token mean riding on the block stack's node, supernet_transformer.py:147-172) against the same
    model with the ends evaluated by the framework: pooled features and every parameter gradient, incl. exactly
    zero gradient outside the sampled width."""
    from cream_amd.autoformer import engine, supernet as SN
    torch.manual_seed(3)
    model = engine.build_supernet("S", drop_path_rate=0.0).to(DEV)
    cfg = dict(layer_num=2, embed_dim=[384] * 2, mlp_ratio=[3.5, 4.0], num_heads=[6, 5])
    model.set_sample_config(cfg)
    model.train()
    x = torch.randn(8, 3, 224, 224, device=DEV)
    gy = torch.randn(8, 384, device=DEV)
    res = {}
    for native in (False, True):
        SN.NATIVE_ENDS = native
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = model.forward_features(x)
        y.backward(gy)
        names = ["patch_embed_super.proj.weight", "patch_embed_super.proj.bias", "cls_token", "pos_embed", "norm.weight",
                 "norm.bias", "blocks.0.fc1.weight", "blocks.1.attn.qkv.weight", "blocks.0.attn_layer_norm.weight"]
        prm = dict(model.named_parameters())
        res[native] = [y.detach().float().clone()] + [prm[n].grad.detach().clone() for n in names]
    SN.NATIVE_ENDS = True
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))        # noqa: E731
    errs = {n: rel(a, b) for n, a, b in zip(["y"] + names, res[True], res[False])}
    print("[native ends]", {k: f"{v:.1e}" for k, v in errs.items()})
    assert res[True][0].dtype == torch.float32 and res[True][0].shape == (8, 384)
    for k, v in errs.items():
        assert v < 2e-2, (k, v)
    prm = dict(model.named_parameters())
    assert float(prm["norm.weight"].grad[384:].abs().max()) == 0.0
    assert float(prm["pos_embed"].grad[..., 384:].abs().max()) == 0.0 and float(prm["cls_token"].grad[..., 384:].abs().max()) == 0.0


def test_hidden_width_not_multiple_of_8_runs_padded_on_the_native_path():
    """supernet-T samples embed_dim 216 with mlp_ratio 3.5 -> a hidden width of 756: the native block pads it to
    760 (the fc1 epilogue writes zeros for the 4 extra hidden units, so every product over them vanishes) instead
    of leaving the fast path.  Against the fp32 module path; gradients of the padding rows / columns exactly zero."""
    from cream_amd.autoformer import engine
    torch.manual_seed(9)
    model = engine.build_supernet("T", drop_path_rate=0.0).to(DEV)
    cfg = dict(layer_num=2, embed_dim=[216] * 2, mlp_ratio=[3.5, 3.5], num_heads=[3, 4])
    model.set_sample_config(cfg)
    model.train()
    assert model.blocks[0].sample_ffn_embed_dim_this_layer == 756
    x = torch.randn(8, 3, 224, 224, device=DEV)
    gy = torch.randn(8, 216, device=DEV)
    ref = model.forward_features(x)                                   # fp32 module path
    ref.backward(gy)
    names = ["blocks.0.fc1.weight", "blocks.0.fc2.weight", "blocks.0.fc1.bias", "blocks.1.attn.qkv.weight", "norm.weight"]
    prm = dict(model.named_parameters())
    want = [prm[n].grad.clone() for n in names]
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = model.forward_features(x)
    assert "StackFunction" in type(y.grad_fn).__name__, "the native block path did not run"
    y.backward(gy)
    rel = lambda a, b: float((a.float() - b).abs().max() / b.abs().max().clamp_min(1e-30))      # noqa: E731
    errs = dict(y=rel(y, ref.detach()), **{n: rel(prm[n].grad, w) for n, w in zip(names, want)})
    print("[F = 756 padded]", {k: f"{v:.1e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < 3e-2, (k, v)
    assert float(prm["blocks.0.fc1.weight"].grad[756:].abs().max()) == 0.0
    assert float(prm["blocks.0.fc2.weight"].grad[:, 756:].abs().max()) == 0.0
    assert float(prm["blocks.0.fc1.bias"].grad[756:].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K,qkv", [(394, 576, 216, True), (197, 1000, 384, False), (25216, 1152, 384, True), (333, 100, 52, False),
                                       (25216, 448, 1792, False)])
def test_fp32_linear_kernels_match_fp64(M, N, K, qkv):
    """csrc/gemm_f32.hip (forward, dgrad, wgrad + bias column sums on v_mfma_f32_32x32x2_f32, the super weight read in place
    through the qkv row map) against the same products in fp64: <= 2e-6 of the largest magnitude for contractions up to
    ~2k terms; the weight / bias gradients at M = 25,216 are ONE sequential fp32 chain over 25,216 tokens per element
    (rounding grows like sqrt(terms) x 6e-8: measured 6.1e-6, bound 2e-5).  Gradients exactly zero outside the active slice."""
    from cream_amd.autoformer import native_fp32
    torch.manual_seed(M + N)
    Ns, Ks = (N + 96 if not qkv else N + 3 * 64), K + 40                    # super extents beyond the sampled ones
    w = (torch.randn(Ns, Ks, device=DEV) * K ** -0.5).requires_grad_()
    b = torch.randn(Ns, device=DEV).requires_grad_()
    x = torch.randn(M, K, device=DEV).requires_grad_()
    gy = torch.randn(M, N, device=DEV)
    seg, step = (N // 3, 3) if qkv else (0, 0)
    y = native_fp32.linear(x, w, b, N, K, seg, step)
    dx, dw, db = torch.autograd.grad(y, [x, w, b], gy)
    rows = torch.arange(N, device=DEV)
    rows = (rows % seg) * step + rows // seg if qkv else rows
    wd, xd, gd = w.detach().double()[rows][:, :K], x.detach().double(), gy.double()
    errs = dict(y=_rel(y.double(), xd @ wd.T + b.detach().double()[:N]), dx=_rel(dx.double(), gd @ wd),
                dw=_rel(dw.double()[rows][:, :K], gd.T @ xd), db=_rel(db.double()[:N], gd.sum(0)))
    print(f"[fp32 own GEMM M={M} N={N} K={K} qkv={qkv}]", {k: f"{v:.1e}" for k, v in errs.items()})
    tol = dict(y=2e-6, dx=2e-6 if N < 1500 else 4e-6, dw=2e-6 if M < 2000 else 2e-5, db=2e-6 if M < 2000 else 2e-5)
    assert all(errs[k] < tol[k] for k in errs), errs
    mask = torch.ones_like(dw, dtype=torch.bool)
    mask[rows[:, None], torch.arange(K, device=DEV)[None, :]] = False
    assert torch.count_nonzero(dw[mask]) == 0 and torch.count_nonzero(db[N:]) == 0


@pytest.mark.parametrize("M,E,Es", [(394, 216, 256), (25216, 384, 448), (197, 448, 448)])
def test_fp32_layernorm_kernels_match_fp64(M, E, Es):
    """The fp32 instantiation of the LayerNorm kernels (csrc/block_ops.hip, Io4<float>) against fp64."""
    from cream_amd.autoformer import native_fp32
    torch.manual_seed(E)
    g = (1 + 0.1 * torch.randn(Es, device=DEV)).requires_grad_()
    b = (0.1 * torch.randn(Es, device=DEV)).requires_grad_()
    x = (torch.randn(M, E, device=DEV) * 2 + 0.5).requires_grad_()
    gy = torch.randn(M, E, device=DEV)
    y = native_fp32.layer_norm(x, g, b, E, 1e-5)
    dx, dg, db = torch.autograd.grad(y, [x, g, b], gy)
    xd = x.detach().double().requires_grad_()
    gd, bd = g.detach().double().requires_grad_(), b.detach().double().requires_grad_()
    yr = torch.nn.functional.layer_norm(xd, (E,), gd[:E], bd[:E], 1e-5)
    rdx, rdg, rdb = torch.autograd.grad(yr, [xd, gd, bd], gy.double())
    errs = dict(y=_rel(y.double(), yr), dx=_rel(dx.double(), rdx), dg=_rel(dg.double(), rdg), db=_rel(db.double(), rdb))
    print(f"[fp32 own LayerNorm M={M} E={E}]", {k: f"{v:.1e}" for k, v in errs.items()})
    assert all(v < 5e-6 for v in errs.values()), errs
    assert torch.count_nonzero(dg[E:]) == 0 and torch.count_nonzero(db[E:]) == 0


def test_bf16_partial_tiles_of_the_weight_gradients_stay_within_their_rounding():
    """cream_block_wgrad_bf16: the split-K partial tiles leave the weight-gradient GEMMs as bf16 (half of the 226 MB of
    partial traffic per block).  Against fp32 partials on the same B = 128 block: every other gradient bit-identical (the
    switch touches nothing else), the four weight gradients within 4e-3 relative L2 (measured 1.9e-3: each of the 8-16
    partial sums is rounded once, as torch.autocast rounds the whole bf16 weight gradient once), bit-reproducible."""
    from cream_amd import _lib
    from cream_amd.autoformer import engine
    torch.manual_seed(0)
    m = engine.build_supernet("S", drop_path_rate=0.0, depth=2).to(DEV)
    m.set_sample_config(dict(layer_num=2, embed_dim=[384] * 2, num_heads=[6, 5], mlp_ratio=[3.5, 4.0]))
    m.train()
    x = torch.randn(128, 3, 224, 224, device=DEV)
    t = torch.softmax(torch.randn(128, 1000, device=DEV), -1)
    lib = _lib.load()
    was = lib.cream_block_wgrad_bf16(-1)
    res = {}
    try:
        for mode in (0, 1, 1):
            lib.cream_block_wgrad_bf16(mode)
            m.zero_grad(set_to_none=False)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = engine.soft_target_cross_entropy(m(x), t)
            loss.backward()
            torch.cuda.synchronize()
            res.setdefault(mode, []).append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    finally:
        lib.cream_block_wgrad_bf16(was)
    worst = 0.0
    big = ("attn.qkv.weight", "attn.proj.weight", "fc1.weight", "fc2.weight")
    for k, a in res[0][0].items():
        b = res[1][0][k]
        assert torch.equal(res[1][1][k], b), k                     # reproducible
        if k.startswith("blocks.") and k.endswith(big):
            worst = max(worst, _rel(b, a))
        else:
            assert torch.equal(a, b), k
    print(f"[bf16 vs fp32 partial tiles of the weight gradients] worst rel difference {worst:.2e}")
    assert 0.0 < worst < 4e-3


def test_block_under_the_multi_gpu_cu_reserve_equals_the_full_grid():
    """cream_cu_reserve(comm.DEFAULT_COMM_CUS) — what every multi-GPU run sets — against reserve 0 on the small two-block model:
    the persistent grids shrink and the token slices of the weight gradients (= the backward workspace layout, cream_block_layout_epoch)
    change.  Per-element arithmetic does not depend on the grid: outputs, dx and every gradient that is no split-K weight gradient are
    bit-identical; the four weight gradients per block differ by the rounding of other partial tiles (the 4e-3 of
    test_bf16_partial_tiles_of_the_weight_gradients_stay_within_their_rounding).  The qkv bias gradient is split-K too: its fp32 partials
    (column sums of dqkv per token slice) ride on the qkv weight-gradient kernel (csrc/block_seq.cpp), so other slices add the same terms
    in another order — the 1e-5 of test_block_stack_equals_block_by_block_with_drop_path for summation-order noise.  A workspace laid out
    for the other budget would show here."""
    from cream_amd import _lib, comm
    from cream_amd.autoformer import block as K
    lib = _lib.load()
    m = _supernet().to(DEV)
    m.set_sample_config(dict(layer_num=2, embed_dim=[384, 384], num_heads=[6, 5], mlp_ratio=[3.5, 3.0]))
    m.train()
    g = torch.Generator(device=DEV).manual_seed(13)
    B = 8
    x0 = torch.randn(B, 197, 384, device=DEV, generator=g)
    dout = torch.randn(B, 197, 384, device=DEV, generator=g)
    blks = list(m.blocks)
    res, splits = [], []
    prev = lib.cream_cu_reserve(-1)
    try:
        for reserve in (0, comm.DEFAULT_COMM_CUS, 0):
            lib.cream_cu_reserve(reserve)
            splits.append(K._wgrad_splits(B * 197, 3 * 320, 384, False, K.wgrad_parts_dtype()))      # block 1's qkv weight gradient
            m.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_()
            y = K.StackFunction.apply(x, None, blks)
            y.backward(dout)
            torch.cuda.synchronize()
            res.append((y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    finally:
        lib.cream_cu_reserve(prev)
    assert splits[0] != splits[1], "the token slices did not follow the budget: the case tests nothing"
    big = ("attn.qkv.weight", "attn.proj.weight", "fc1.weight", "fc2.weight")
    for other in (1, 2):                                           # reserve 16, and back at 0 (the epoch moved twice)
        assert torch.equal(res[0][0], res[other][0]) and torch.equal(res[0][1], res[other][1])
        assert set(res[0][2]) == set(res[other][2]) and len(res[0][2]) >= 2 * 16
        for k, v in res[0][2].items():
            assert torch.isfinite(res[other][2][k]).all(), k
            if other == 1 and k.endswith(big):
                assert _rel(res[other][2][k], v) < 4e-3, k
            elif other == 1 and k.endswith("attn.qkv.bias"):
                assert _rel(res[other][2][k], v) < 1e-5, k
            else:
                assert torch.equal(res[other][2][k], v), k


@pytest.mark.parametrize("B,C,dt", [(128, 1000, torch.bfloat16), (5, 1000, torch.float32), (16, 2048, torch.bfloat16), (3, 37, torch.float32)])
def test_soft_target_ce_kernel_matches_torch(B, C, dt):
    """cream_soft_ce (loss rows + logit gradient in one launch) against the framework formulation of
    timm.loss.SoftTargetCrossEntropy in fp64 on the same (rounded) logits: loss and d loss / d logits, also under an
    incoming gradient != 1 and with unnormalised targets (Mixup's soft labels sum to 1; the kernel does not assume it)."""
    from cream_amd.autoformer import block as K
    torch.manual_seed(B * C)
    logits = (4 * torch.randn(B, C, device=DEV)).to(dt).requires_grad_()
    target = torch.softmax(torch.randn(B, C, device=DEV), -1) * (1.0 + 0.1 * torch.rand(B, 1, device=DEV))
    assert K.soft_ce_supported(logits, target)
    loss = K.SoftTargetCEFunction.apply(logits, target)
    (g,) = torch.autograd.grad(loss, logits, torch.tensor(0.75, device=DEV))
    x = logits.detach().double().requires_grad_()
    ref = torch.sum(-target.double() * torch.log_softmax(x, -1), -1).mean()
    (rg,) = torch.autograd.grad(ref, x, torch.tensor(0.75, device=DEV, dtype=torch.float64))
    el, eg = abs(float(loss) - float(ref)) / abs(float(ref)), _rel(g.double(), rg)
    print(f"[soft CE B={B} C={C} {dt}] loss {el:.1e} dlogits {eg:.1e}")
    assert el < 2e-6 and eg < (4e-3 if dt == torch.bfloat16 else 5e-6)        # bf16: the returned gradient is rounded to bf16
    assert g.dtype == dt


def test_native_head_matches_fp32_linear():
    """The classifier on the own GEMMs (block.HeadFunction: NT forward, dgrad on the transposed copy, weight + bias gradient
    through one TN launch added into the active slice of the .grad tensors) against F.linear in fp32 on the same inputs."""
    from cream_amd.autoformer import block as K, engine
    torch.manual_seed(3)
    m = engine.build_supernet("S", drop_path_rate=0.0, depth=1).to(DEV)
    cfg = dict(layer_num=1, embed_dim=[384], num_heads=[6], mlp_ratio=[3.5])
    m.set_sample_config(cfg)
    feat = torch.randn(128, 384, device=DEV, requires_grad=True)
    gy = torch.randn(128, 1000, device=DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert K.head_supported(m.head, feat)
        y = K.head(m.head, feat)
    m.head.weight.grad = torch.full_like(m.head.weight, 0.5)        # the node ADDS into existing gradients
    m.head.bias.grad = None
    (dx,) = torch.autograd.grad(y, feat, gy.to(torch.bfloat16))
    w, b = m.head.weight.detach()[:, :384], m.head.bias.detach()
    errs = dict(y=_rel(y.float(), feat.detach() @ w.T + b), dx=_rel(dx, gy @ w),
                dw=_rel(m.head.weight.grad[:, :384] - 0.5, gy.T @ feat.detach()), db=_rel(m.head.bias.grad, gy.sum(0)))
    print("[native head]", {k: f"{v:.1e}" for k, v in errs.items()})
    assert all(v < 8e-3 for v in errs.values()), errs                 # bf16 operands (feat, W, dlogits rounded to bf16)
    assert torch.all(m.head.weight.grad[:, 384:] == 0.5)


def test_forward_without_backward_skips_the_gelu_derivative_and_gives_the_same_output():
    """A forward that no backward will follow (no_grad evaluation, a frozen teacher): the fc1 epilogue writes gelu(h) only
    (cream_linear_gelu_fwd with gp = NULL, cream_block_desc.inference) — same outputs bit for bit."""
    from cream_amd.autoformer import block as K
    g_ = torch.Generator(device=DEV).manual_seed(5)
    M, E, F_ = 197 * 4, 384, 1344
    x = torch.randn(M, E, device=DEV, generator=g_).bfloat16()
    w = (torch.randn(F_, E, device=DEV, generator=g_) * E ** -0.5).bfloat16()
    b = torch.randn(F_, device=DEV, generator=g_).bfloat16()
    gp, g = K.linear_gelu_fwd(x, w, b, F_, E)
    gp2, g2 = K.linear_gelu_fwd(x, w, b, F_, E, want_grad=False)
    assert gp2 is None and gp is not None and torch.equal(g, g2)
    m = _supernet(depth=2).to(DEV)
    cfg = dict(layer_num=2, embed_dim=[448] * 2, num_heads=[7, 6], mlp_ratio=[4.0, 3.5])
    m.set_sample_config(cfg)
    m.eval()
    x0 = torch.randn(3, 197, 448, device=DEV, generator=g_)
    blks = list(m.blocks)
    y_grad = K.StackFunction.apply(x0.clone().requires_grad_(), None, blks)
    with torch.no_grad():
        y_eval = K.StackFunction.apply(x0, None, blks)
    torch.cuda.synchronize()
    assert torch.equal(y_grad.detach(), y_eval)


@pytest.mark.parametrize("M,N,K,ldw", [(25216, 1344, 384, 448), (25216, 384, 1344, 1792), (1000, 200, 136, 144),
                                        (197 * 8, 320, 1120, 1792), (197 * 8, 448, 448, 448)])
def test_phase_interleaved_nt_kernel_matches_fp32_and_the_two_stage_kernels(M, N, K, ldw):
    """csrc/gemm_nt8.hpp (cream_gemm_nt8(1): 256 x 256 tile, counted vmcnt, two staggered wave rows, K-tile stream continuous over the
    output tiles, per-wave epilogue) against plain PyTorch fp32 of the same products (Linear_super.py:38-54, :71-81) and against
    the two-stage kernels on the same inputs: forward, forward without bias, dgrad, bias + GELU (both outputs) and the
    x gelu' dgrad with its column sums — row / column edges, K tails (136, 1120 % 64 != 0), several tiles per workgroup
    (594 at the bench shape), and twice in a row (every launch of a sync-structure change is checked)."""
    from cream_amd import _lib
    from cream_amd.autoformer import block as K_
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    wsup = (torch.randn(N + 64, ldw, device=DEV, generator=g) * 0.05).bfloat16()
    bias = torch.randn(N + 64, device=DEV, generator=g).bfloat16()
    dy = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    gp = torch.rand(M, K, device=DEV, generator=g).bfloat16()
    W = wsup[:N, :K].float()
    wt = torch.zeros(ldw, N + 64, device=DEV, dtype=torch.bfloat16)
    wt[:, :] = wsup.t()

    def run():
        out = K_.linear_fwd(x, wsup, bias, N, K)
        out0 = K_.linear_fwd(x, wsup, None, N, K)
        dx = K_.linear_dgrad(dy, wt, N, K)
        gpo, go = K_.linear_gelu_fwd(x, wsup, bias, N, K)
        dh, cs = K_.linear_dgrad_mul(dy, wt, gp, N, K)
        return out, out0, dx, gpo, go, dh, cs

    was = lib.cream_gemm_nt8(-1)
    try:
        lib.cream_gemm_nt8(0)
        ref = run()
        lib.cream_gemm_nt8(1)
        new = run()
        again = run()
    finally:
        lib.cream_gemm_nt8(was)
    for a, b in zip(new, again):
        assert torch.equal(a, b)                                           # reproducible (no race between the staggered wave rows)
    out, out0, dx, gpo, go, dh, cs = new
    assert _rel(out.float(), x.float() @ W.t() + bias[:N].float()) < 1e-2
    assert _rel(out0.float(), x.float() @ W.t()) < 1e-2
    assert _rel(dx.float(), dy.float() @ W) < 1e-2
    # same products, same accumulation order over K, one rounding: the plain / bias / GELU epilogues agree with the two-stage
    # kernels to the last bit
    for a, b in zip(new[:5], ref[:5]):
        assert torch.equal(a, b)
    # x gelu': this kernel rounds dy . W to bf16 before the multiplication (as the reference's two operators do), the two-stage
    # kernel multiplies the fp32 accumulator: one bf16 ulp apart at most, both within 1e-2 of fp32
    want = (dy.float() @ W) * gp.float()
    assert _rel(dh.float(), want) < 1e-2 and _rel(dh.float(), ref[5].float()) < 1e-2
    two_step = ((dy.float() @ W).bfloat16().float() * gp.float()).bfloat16()
    assert float((dh.float() - two_step.float()).abs().max()) <= 2 ** -7 * float(two_step.float().abs().max())
    assert cs.shape == ref[6].shape and _rel(cs.sum(0), dh.float().sum(0)) < 1e-5


@pytest.mark.parametrize("M,N,K", [(25216, 1344, 384), (25216, 384, 1344), (25216, 1152, 448), (25216, 320, 320), (1000, 328, 264), (394, 200, 136)])
def test_macro_tile_weight_gradient_kernel_writes_correctly_rounded_partial_tiles(M, N, K):
    """csrc/gemm_tn8.hpp (cream_linear_wgrad_parts_bf16 called with cream_linear_wgrad_splits_bf16's split count): every bf16
    partial tile equals the fp32 sum of dy_s^T x_s over ITS token slice rounded once (within one bf16 ulp of the fp64 value), the bias
    partials add up to the column sums of dy (Linear_super.py:71-81 backward), tiles that stick out of the matrix (N, K not
    multiples of 256, blocks of 8 columns), token tails (M % 64 != 0), and the 128 x 128 kernel called with the SAME split count
    writes the same tiles (<= 1 bf16 ulp: same slices, different tile shape)."""
    import ctypes
    from cream_amd import _lib
    from cream_amd.autoformer import block as K_
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(12)
    dy = (torch.randn(M, N, device=DEV, generator=g) * 0.1).bfloat16()
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    was = lib.cream_gemm_tn8(-1)
    try:
        lib.cream_gemm_tn8(2)
        S = lib.cream_linear_wgrad_splits_bf16(M, N, K)
        parts, bparts = K_.linear_wgrad_parts(dy, x, want_bias=True, parts_dtype=torch.bfloat16)
        parts2, _ = K_.linear_wgrad_parts(dy, x, want_bias=False, parts_dtype=torch.bfloat16)
        assert parts.shape == (S, N, K) and parts.dtype == torch.bfloat16 and bparts.shape == (S, N)
        assert torch.equal(parts, parts2)                                  # bias partials ride along: same tiles; reproducible
        lib.cream_gemm_tn8(0)                                              # the 128 x 128 kernel with the same S
        old = torch.empty_like(parts)
        _lib.check(lib.cream_linear_wgrad_parts_bf16(old.data_ptr(), ctypes.c_void_p(0), dy.data_ptr(), x.data_ptr(), M, N, K, S,
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "cream_linear_wgrad_parts_bf16")
    finally:
        lib.cream_gemm_tn8(was)
    steps = (M + 63) // 64
    worst = 0.0
    for s in range(S):
        lo, hi = steps * s // S * 64, min(M, steps * (s + 1) // S * 64)
        want = dy[lo:hi].double().t() @ x[lo:hi].double()
        err = (parts[s].double() - want).abs()
        assert bool((err <= want.abs() * 2.0 ** -8 + 1e-3).all()), s       # one rounding to bf16 (+ fp32 accumulation noise)
        worst = max(worst, float((parts[s].float() - old[s].float()).abs().max() / want.abs().max()))
    assert worst <= 2.0 ** -7
    assert _rel(bparts.sum(0), dy.float().sum(0)) < 1e-4
    assert _rel(parts.float().sum(0), dy.float().t() @ x.float()) < 4e-3


@pytest.mark.parametrize("M,N,K,ldw", [(25216, 384, 1536, 1792), (25216, 320, 960, 1792), (25216, 384, 384, 448), (197 * 8, 320, 320, 448),
                                        (1000 + 24, 384, 200, 208), (2048 + 8, 320, 136, 144)])
def test_256x192_nt_tile_matches_fp32_and_the_other_tiles(M, N, K, ldw):
    """csrc/gemm_mfma.hip launch_nt_half (cream_gemm_nthalf(1), round 6): the 256 x 192 tile — column tiles that are no power of two
    (rotated fp32 staging rows, 504 of 512 epilogue threads, ragged DMA pieces) — for the plain / bias products whose output is
    384 or 320 wide (Linear_super.py:38-54, :71-81: proj, fc2, the input gradients of fc1 / qkv / proj): against plain PyTorch fp32
    and, bit for bit, against the tiles chosen without it; row edges (M % 256 != 0), the 192 + 128 split of N = 320, K tails
    (200, 136 % 64 != 0), twice in a row."""
    from cream_amd import _lib
    from cream_amd.autoformer import block as K_
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(23)
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    wsup = (torch.randn(N + 64, ldw, device=DEV, generator=g) * 0.05).bfloat16()
    bias = torch.randn(N + 64, device=DEV, generator=g).bfloat16()
    dy = torch.randn(M, K, device=DEV, generator=g).bfloat16()            # gradient of an (M, K)-wide output: dx = dy . W^T is N wide
    W = wsup[:N, :K].float()

    def run():
        out = K_.linear_fwd(x, wsup, bias, N, K)                           # EPI_BIAS, N wide
        out0 = K_.linear_fwd(x, wsup, None, N, K)
        # dgrad with an N-wide result: dx (M x N) = dy (M x K) . Wt^T with Wt = wsup[:N, :K] as the (N x K) "transposed copy"
        dx = K_.linear_dgrad(dy, wsup, K, N)                               # EPI_STORE, N wide
        return out, out0, dx

    was = lib.cream_gemm_nthalf(-1)
    try:
        lib.cream_gemm_nthalf(0)
        ref = run()
        lib.cream_gemm_nthalf(1)
        new = run()
        again = run()
    finally:
        lib.cream_gemm_nthalf(was)
    for a, b in zip(new, again):
        assert torch.equal(a, b)
    out, out0, dx = new
    assert _rel(out.float(), x.float() @ W.t() + bias[:N].float()) < 1e-2
    assert _rel(out0.float(), x.float() @ W.t()) < 1e-2
    assert _rel(dx.float(), dy.float() @ W.t()) < 1e-2
    for a, b in zip(new, ref):                                             # same contraction order per element, one rounding
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,N,K,ldw", [(25216, 1344, 384, 448), (25216, 960, 320, 448), (1000 + 24, 704, 200, 208), (197 * 3, 1792, 448, 448)])
def test_nt_epilogue_variants_are_bit_identical(M, N, K, ldw):
    """csrc/gemm_mfma.hpp "OPT" (cream_gemm_ntopt, round 6): the 128-wide two-stage NT kernels with the tile epilogue off the memory
    counters (asm LDS-DMA, LDS-only barriers, side inputs under the first K-step, counted vmcnt behind an epilogue: bit 0) and
    gelu / gelu' from the 16 KB LDS table (bit 1) — against the kernels without them, bit for bit, on the fc1 + GELU epilogue
    (gelu and gelu'), the x gelu' epilogue with its column sums and the bias epilogue (Linear_super.py:71-81,
    supernet_transformer.py:275-285): full tiles, row / column edges, a K tail, biases that push h out of the table's range."""
    from cream_amd import _lib
    from cream_amd.autoformer import block as K_
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    wsup = (torch.randn(N + 64, ldw, device=DEV, generator=g) * 0.05).bfloat16()
    bias = torch.randn(N + 64, device=DEV, generator=g)
    bias[5], bias[6], bias[7], bias[N - 1] = 40.0, -40.0, 0.0, 17.0            # |h| >= 16: the direct evaluation of the wave's chunk
    bias = bias.bfloat16()
    x[3].zero_()                                                               # h = bias exactly in one row
    dy = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    fac = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    wt = (torch.randn(N + 64, ldw, device=DEV, generator=g) * 0.05).bfloat16()    # (in = N rows, out = K) transposed copy for the dgrad

    def run():
        gp, ge = K_.linear_gelu_fwd(x, wsup, bias, N, K)
        _, ge_only = K_.linear_gelu_fwd(x, wsup, bias, N, K, want_grad=False)
        out = K_.linear_fwd(x, wsup, bias, N, K)
        dh, parts = K_.linear_dgrad_mul(dy, wt, fac, K, N)                       # dh (M, N) = (dy (M, K) . W) * fac
        return gp, ge, ge_only, out, dh, parts

    was = lib.cream_gemm_ntopt(-1)
    try:
        lib.cream_gemm_ntopt(0)
        ref = run()
        res = {}
        for mode in (1, 3, 9, 11, 11):          # bit 3: the backward's epilogues (x gelu', plain store) as well
            lib.cream_gemm_ntopt(mode)
            res.setdefault(mode, []).append(run())
    finally:
        lib.cream_gemm_ntopt(was)
    for mode in (1, 3, 9, 11):
        for a, b in zip(res[mode][0], ref):
            assert torch.equal(a, b), mode
    for a, b in zip(res[11][1], ref):
        assert torch.equal(a, b)
    assert torch.equal(ref[1], ref[2])
    h = (x.float() @ wsup[:N, :K].float().t() + bias[:N].float())
    assert _rel(ref[1].float(), torch.nn.functional.gelu(h)) < 1e-2


def test_gelu_table_epilogue_over_every_bf16_value():
    """The table path of the fc1 + GELU epilogue (csrc/gemm_mfma.hpp, OPT & 2) against the direct evaluation over EVERY finite bf16
    value of h — x rows are unit vectors, so h = a weight entry exactly — plus inf / nan / denormals through the bias:
    bit-identical gelu(h) and gelu'(h), except |h| < 2^-125 (gelu = h / 2 as an exponent decrement: differs by < 1.2e-38)."""
    from cream_amd import _lib
    from cream_amd.autoformer import block as K_
    lib = _lib.load()
    pats = torch.arange(65536, dtype=torch.int32, device=DEV)
    finite = pats[((pats >> 7) & 0xFF) != 0xFF]                                 # 65,280 patterns
    N, K, M = finite.numel() // 8, 8, 256
    w = finite.to(torch.int16).view(torch.bfloat16).view(N, K).contiguous()
    x = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    x[torch.arange(M, device=DEV), torch.arange(M, device=DEV) % 8] = 1.0
    bias0 = torch.zeros(N, device=DEV, dtype=torch.bfloat16)
    spec = torch.tensor([0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x8001, 0x007F, 0x0080, 0x00FF, 0x0100, 0x8100, 0x3980, 0xB980, 0x397F, 0x417F, 0x4180, 0xC180],
                        dtype=torch.int32, device=DEV).to(torch.int16).view(torch.bfloat16)
    N2 = 640
    bias2 = spec.repeat(N2 // spec.numel())
    w2 = torch.zeros(N2, K, device=DEV, dtype=torch.bfloat16)

    def run():
        return K_.linear_gelu_fwd(x, w, bias0, N, K) + K_.linear_gelu_fwd(x, w2, bias2, N2, K)

    was = lib.cream_gemm_ntopt(-1)
    try:
        lib.cream_gemm_ntopt(0)
        ref = run()
        lib.cream_gemm_ntopt(3)
        new = run()
    finally:
        lib.cream_gemm_ntopt(was)
    for i, (a, b) in enumerate(zip(new, ref)):
        ai, bi = a.view(torch.int16), b.view(torch.int16)
        same = (ai == bi) | (a.isnan() & b.isnan())
        if same.all():
            continue
        # the documented exception: |h| < 2^-125 (bit patterns 0x0001 .. 0x00FF): both results below 1.2e-38
        bad = ~same
        assert (a[bad].float().abs() < 1.2e-38).all() and (b[bad].float().abs() < 1.2e-38).all(), (i, int(bad.sum()))
    # (every finite pattern really went through: row m of the first product is the weight column m % 8 — within the fast erf's error)
    want = torch.nn.functional.gelu(w.float())
    got = ref[1][:8].float().t()
    ok = torch.isfinite(want)
    assert ((got - want)[ok].abs() <= 1e-2 * want[ok].abs() + 1e-6).all()
