"""`finetune_step` (cream_amd/tinyvit_finetune.py) on the device: the small TinyViT of the fixtures, B = 2, drop-path 0, bf16
autocast, base rate 1e-2, weight decay 1e-8, layer_lr_decay 0.8, NativeAdamW with the recipe's ten groups.  The first-step
property and its derived bound are those of tests/test_tinyvit_finetune.py, which checks on the CPU that the reference
arithmetic (torch.optim.AdamW) stays inside the bound and above the element floor on the same inputs."""
import math

import pytest
import torch

from test_tinyvit_finetune import (FLOOR, STEP_LR, WEIGHT_DECAY, WarmupCosine, batch, bn_state, build, capture_gradients,
                                   check_first_step, ulp32)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _setup():
    from cream_amd import tinyvit_finetune as FT
    from cream_amd.autoformer import engine
    model = build().to(DEV)
    opt = FT.build_finetune_optimizer(model, STEP_LR, weight_decay=WEIGHT_DECAY)
    assert isinstance(opt, engine.NativeAdamW) and len(opt.param_groups) == 10
    sched = FT.LRSchedulerWrapper(WarmupCosine(opt, STEP_LR), opt)
    sched.step_update(4)                                                     # end of warm-up: STEP_LR x lr_scale
    rates = [g['lr'] for g in opt.param_groups]
    assert rates == [STEP_LR * g['lr_scale'] for g in opt.param_groups] and len(set(rates)) == 5
    return FT, model, opt, sched, rates


def test_first_step_moves_every_parameter_by_its_own_groups_rate():
    from cream_amd import timing, tinyvit
    FT, model, opt, sched, rates = _setup()
    stats = bn_state(model)
    before = {p: p.detach().clone() for p in model.parameters()}
    grads = capture_gradients(opt)
    blocks = [b for layer in model.layers[1:] for b in layer.blocks]
    calls = []
    hooks = [b.local_conv.c.register_forward_hook(lambda *a: calls.append("conv")) for b in blocks]
    folded = tinyvit.TinyViTBlock._folded
    tinyvit.TinyViTBlock._folded = lambda self: (calls.append("folded"), folded(self))[1]
    timing.reset()
    timing.enable(True)
    try:
        x, y = batch(DEV)
        out = FT.finetune_step(model, opt, x, y, max_norm=5.0, index=0, lr_scheduler=sched)
        torch.cuda.synchronize()
    finally:
        timing.enable(False)
        tinyvit.TinyViTBlock._folded = folded
        for h in hooks:
            h.remove()
    # the route: BatchNorm in eval mode inside a training model, the folded one-launch convolution through autograd
    s = timing.summary()
    assert calls == ["folded"] * len(blocks) and s["token_dwconv3_fwd"]["launches"] == s["token_dwconv3_bwd"]["launches"] == len(blocks)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert bns and not any(m.training for m in bns)
    assert all(m.training for m in model.modules() if not isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
    now = bn_state(model)
    assert stats and all(torch.equal(now[k], v) for k, v in stats.items())
    # the step
    norm = float(out['grad_norm'])
    coef = float(torch.tensor(min(1.0, 5.0 / (norm + 1e-6)), dtype=torch.float32))
    print(f"\n[tinyvit finetune gpu] loss {out['loss']:.4f} grad norm {norm:.4f} coef {coef:.4f}", end="")
    assert math.isfinite(out['loss']) and norm > 0 and out['grad_norm'] is opt.grad_norm
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in model.parameters())   # zeroed, tensors kept
    assert sched.lr_scheduler.last == 0 and opt._steps == 1
    check_first_step(opt, rates, before, grads, coef, tag="gpu NativeAdamW")
    # ... and a parameter of the deepest group did NOT move by the head's rate
    p = next(p for p in opt.param_groups[0]['params'] if float(grads[p].abs().max()) * coef >= 2 * FLOOR)
    g = grads[p].double().cpu() * coef
    dp = (p.detach().double().cpu() - before[p].double().cpu()).abs()[g.abs() >= FLOOR]
    assert float((dp / rates[4] - 1.0).abs().min()) > 0.5


def test_accumulation_updates_on_the_last_call_with_the_summed_gradient():
    """accumulation_steps = 2: the first call changes no parameter and keeps the gradients, the second updates; the result is one
    step on the summed half-losses.  The two gradients differ only by the rounding of the fp32 sum (each element one rounding,
    relative 2^-24, in either order) — through the norm into the coefficient likewise —, and the update g' / (|g'| + eps) moves
    by at most a quarter of the relative change of g' (its derivative eps / (|g'| + eps)^2 times |g'| is at most 1 / 4): per
    element |dp| <= lr_g * 2^-23 + 2 ulp(max|p|), taken generously."""
    from cream_amd import tinyvit_finetune as FT
    _, model, opt, sched, rates = _setup()
    _, twin, opt_t, _, rates_t = _setup()
    assert rates == rates_t
    xa, ya = batch(DEV)
    xb, yb = batch(DEV, 'second')
    before = [p.detach().clone() for p in model.parameters()]
    out = FT.finetune_step(model, opt, xa, ya, max_norm=5.0, accumulation_steps=2, index=0, lr_scheduler=sched)
    assert out['grad_norm'] is None and opt._steps == 0 and sched.lr_scheduler.last == 4
    assert all(torch.equal(p, b) for p, b in zip(model.parameters(), before))
    first = [p.grad.clone() for p in model.parameters()]
    assert all(float(g.abs().max()) > 0 for g in first)
    grads = capture_gradients(opt)
    out = FT.finetune_step(model, opt, xb, yb, max_norm=5.0, accumulation_steps=2, index=1, lr_scheduler=sched)
    assert out['grad_norm'] is not None and opt._steps == 1 and sched.lr_scheduler.last == 0
    assert any(not torch.equal(grads[p], f) for p, f in zip(model.parameters(), first))         # the second gradient was added
    # the twin: one backward of the summed half-losses, one step
    twin.train()
    FT.set_bn_state(twin)
    # (one autocast region per forward, as in two calls: inside ONE region the bf16 copy of a weight is cached and shared, and
    # the two gradients of that copy would be added in bf16 before they reach the fp32 parameter)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        la = FT.label_smoothing_cross_entropy(twin(xa), ya) / 2
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lb = FT.label_smoothing_cross_entropy(twin(xb), yb) / 2
    (la + lb).backward()
    opt_t.step(max_norm=5.0)
    torch.cuda.synchronize()
    worst, same, twins = 0.0, 0, dict(twin.named_parameters())
    for group, lr in zip(opt.param_groups, rates):
        for p in group['params']:
            q = twins[p.param_name]
            bound = lr * 2.0 ** -23 + 2.0 * ulp32(max(float(q.detach().abs().max()), 1e-30))
            err = float((p.detach() - q.detach()).abs().max())
            worst, same = max(worst, err / bound), same + int(err == 0.0)
            assert err <= bound, (p.param_name, err, bound)
    print(f"\n[tinyvit finetune gpu] accumulation against the summed loss: worst error / bound {worst:.3f}, {same} of {len(twins)} "
          f"parameters bit-identical", end="")
