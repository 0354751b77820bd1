"""TinyViT on the streaming window attention (cream_amd/window_attn_xl.py, windows of 15 .. 32) on the GPU:
A. one block at w = 16 (four windows) and at w = 24 (one 576-token window) against its own composed branch — fp32 composed as the
   reference, bf16 composed as the yardstick of bf16 noise (the rule of tests/test_efficientvit_gpu.py),
B. eval mode uses the table cached when training mode was left (the reference's quirk),
C. a small whole model whose middle stage is one 256-token window per image: a forward, a backward and an optimizer step."""
from contextlib import nullcontext

import pytest
import torch

from helpers import max_rel
from test_tinyvit_gpu import CONV, LARGE, SMALL, attention_fused_off, case_inputs, composed, make_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
XL = {"window_attn_xl_fwd", "window_attn_xl_bwd"}

CASES = {
    "w16_four_windows": dict(H=2, res=(32, 32), window=16, B=2),
    "w24_single": dict(H=3, res=(24, 24), window=24, B=1),
}


def run_block(blk, x, gy, autocast, fused):
    """-> ({name: tensor}, regions seen, softmax calls of the composed attention)"""
    from cream_amd import timing
    blk.train()
    blk.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    calls = []
    hook = blk.attn.softmax.register_forward_hook(lambda *a: calls.append(1))
    timing.reset()
    timing.enable(True)
    try:
        with (nullcontext() if fused else composed([blk])), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = blk(x)
        (y.float() * gy).sum().backward()
    finally:
        timing.enable(False)
        hook.remove()
    res = {"out": y, "dx": x.grad, "d qkv.weight": blk.attn.qkv.weight.grad, "d attention_biases": blk.attn.attention_biases.grad,
           "d proj.weight": blk.attn.proj.weight.grad}
    return {k: v.detach().float().cpu() for k, v in res.items()}, set(timing.summary()), len(calls)


@pytest.mark.parametrize("tag", list(CASES))
def test_block_fused_against_composed(tag):
    """err(fused) <= max(2 err(composed bf16), 2^-7) for out, dx, d qkv.weight, d attention_biases and d proj.weight, both against
    the fp32 composed path; the regions and the hook say which code ran."""
    c = CASES[tag]
    blk = make_block(c)
    x, gy = case_inputs(c)
    ref, names_a, soft_a = run_block(blk, x, gy, autocast=False, fused=False)
    comp, names_b, soft_b = run_block(blk, x, gy, autocast=True, fused=False)
    fus, names_c, soft_c = run_block(blk, x, gy, autocast=True, fused=True)
    assert not (XL | LARGE | SMALL) & (names_a | names_b) and (soft_a, soft_b) == (1, 1), (names_a, names_b)
    assert XL | CONV <= names_c and not (LARGE | SMALL) & names_c and soft_c == 0, names_c
    bad = []
    for k in ref:
        eb, ec = max_rel(comp[k], ref[k]), max_rel(fus[k], ref[k])
        bound = max(2 * eb, 2.0 ** -7)
        print(f"[tinyvit xl block {tag}] {k:22s} composed bf16 {eb:.3e}  fused {ec:.3e}  bound {bound:.3e}")
        if not ec <= bound:
            bad.append((k, eb, ec))
    assert not bad, bad


def test_eval_mode_uses_the_cached_table():
    from cream_amd import timing
    c = CASES["w16_four_windows"]
    blk = make_block(c).eval()
    x, _ = case_inputs(c)

    def run():
        timing.reset()
        timing.enable(True)
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                y = blk(x)
        finally:
            timing.enable(False)
        assert "window_attn_xl_fwd" in timing.summary() and "window_attn_xl_bwd" not in timing.summary()
        return y.float().cpu()

    y1 = run()
    with torch.no_grad():
        blk.attn.attention_biases.add_(1.0 + torch.arange(256, device=DEV).view(1, -1) / 64)
    assert torch.equal(run(), y1)                                 # stale until training mode is left again
    blk.train()
    blk.eval()
    y3 = run()
    assert not torch.equal(y3, y1)
    with attention_fused_off(), torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        comp = blk(x).float().cpu()
    with composed([blk]), torch.no_grad():
        ref = blk(x).float().cpu()
    eb, ec = max_rel(comp, ref), max_rel(y3, ref)
    print(f"[tinyvit xl eval] composed bf16 {eb:.3e}  fused {ec:.3e}")
    assert ec <= max(2 * eb, 2.0 ** -7)


MODEL = dict(img_size=128, num_classes=10, embed_dims=[32, 64, 96], depths=[1, 2, 2], num_heads=[1, 2, 3], window_sizes=[7, 16, 8])


def test_whole_model_step_with_a_256_token_middle_stage():
    """Stage 1 of this model is one 16 x 16 window per image (xl), stage 2 one 8 x 8 window (small).  Logits, and the root mean
    square and the maximum of the per-parameter gradient deviations and of the optimizer step's deviations, fused against
    composed bf16, both measured against the fp32 composed run: fused <= max(2 composed, 2^-7).  This model in training mode at
    B = 4 amplifies bf16 noise on either path (measured: logits 0.134 fused, 0.127 composed bf16; gradient deviations rms 0.304
    and 0.303), so the figures say that the two bf16 paths are equally far from fp32; which code ran is what the hooks and the
    regions decide.  The block test above is the sharp one."""
    from test_tinyvit import ZERO, build
    from cream_amd import timing
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 128, 128, generator=g).to(DEV)
    gy = torch.randn(4, 10, generator=g).to(DEV)
    blocks = lambda m: [b for layer in m.layers[1:] for b in layer.blocks]          # noqa: E731

    def step(autocast, fused):
        model = build(MODEL).to(DEV).train()
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        calls = []
        hooks = [b.attn.softmax.register_forward_hook(lambda *a: calls.append(1)) for b in blocks(model)]
        timing.reset()
        timing.enable(True)
        try:
            with (nullcontext() if fused else composed(blocks(model))), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                logits = model(x)
            (logits.float() * gy).sum().backward()
            opt.step()
        finally:
            timing.enable(False)
            for h in hooks:
                h.remove()
        grads = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
        moved = {k: (p.detach() - before[k]).float().cpu() for k, p in model.named_parameters()}
        return logits.detach().float().cpu(), grads, moved, timing.summary(), len(calls)

    ref = step(False, False)
    comp = step(True, False)
    fus = step(True, True)
    assert ref[4] == comp[4] == 4 and fus[4] == 0 and not (XL | SMALL | LARGE) & (set(ref[3]) | set(comp[3]))
    s = fus[3]
    assert XL | SMALL <= set(s) and not LARGE & set(s), set(s)
    assert s["window_attn_xl_fwd"]["launches"] == 2 and s["window_attn_xl_bwd"]["launches"] == 2, s
    el_c, el_f = max_rel(comp[0], ref[0]), max_rel(fus[0], ref[0])
    print(f"[tinyvit xl model] logits: composed {el_c:.3e} fused {el_f:.3e}")
    assert el_f <= max(2 * el_c, 2.0 ** -7)
    rms = lambda v: (sum(t * t for t in v) / len(v)) ** 0.5          # noqa: E731
    for what, i in (("gradient", 1), ("step", 2)):
        keys = [k for k in ref[i] if k not in ZERO]                 # zero in exact arithmetic: no relative figure
        fc, ff = [max_rel(comp[i][k], ref[i][k]) for k in keys], [max_rel(fus[i][k], ref[i][k]) for k in keys]
        print(f"[tinyvit xl model] {what} deviations over {len(keys)} parameters: rms composed {rms(fc):.3e} fused {rms(ff):.3e}; "
              f"max composed {max(fc):.3e} fused {max(ff):.3e}")
        assert len(keys) >= 50
        assert rms(ff) <= max(2 * rms(fc), 2.0 ** -7) and max(ff) <= max(2 * max(fc), 2.0 ** -7)
