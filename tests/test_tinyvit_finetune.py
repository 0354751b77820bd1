"""TinyViT's fine-tune recipe (cream_amd/tinyvit_finetune.py) on the CPU: the parameter groups and the schedule against the
reference-made fixture tests/golden/tinyvit_finetune.json, one `finetune_step` with the torch.optim.AdamW that
`build_finetune_optimizer` returns there, and the argument checks of cream_adamw_step_groups (nothing is launched).

The first-step property (shared with tests/test_tinyvit_finetune_gpu.py).  From zero moments the bias-corrected moments of
step 1 are g' and g'^2 (g' the clipped gradient), so AdamW moves an element by
    dp = -lr wd p - lr g' / (|g'| + eps),        | |dp| / lr - 1 | <= eps / |g'| + wd |p| + (rounding)
Over the elements with |g'| >= FLOOR = 1e-4 the bound of a parameter in a group of rate lr_g is the sum of
    eps / FLOOR                     the eps in the denominator
    wd max|p|                       the decoupled weight decay
    2 ulp(max|p|) / lr_g            p is stored in fp32 before and after: two roundings of half an ulp each, and as much again
                                    for the product with the decay factor
    8 * 2^-24                       a few fp32 roundings of the update itself (products, the square root, the division)
— derived, not measured.  A parameter updated with ANOTHER group's rate misses it by the ratio of the rates (>= 0.2 here)."""
import ctypes
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_tinyvit_finetune_golden import BASE_LR, LAYER_LR_DECAY, UPDATES, WEIGHT_DECAY, WarmupCosine  # noqa: E402
from make_tinyvit_golden import MODEL, inputs, tinyvit_fill  # noqa: E402

FLOOR = 1e-4
STEP_LR = 1e-2                                 # the larger rate of the step tests: keeps the ulp term small at 0.8^4
TARGETS = (3, 7)


def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tinyvit_finetune.json")) as fh:
        return json.load(fh)


def build():
    from cream_amd import tinyvit
    torch.manual_seed(0)
    model = tinyvit.TinyViT(**dict(MODEL, layer_lr_decay=LAYER_LR_DECAY))
    tinyvit_fill(model)
    return model


def batch(device, tag='small'):
    return inputs(tag)[0].to(device), torch.tensor(TARGETS, device=device)


def bn_state(model):
    return {k: v.clone() for k, v in model.state_dict().items() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}


def ulp32(x):
    """One fp32 ulp at magnitude x > 0."""
    return 2.0 ** (math.floor(math.log2(x)) - 23)


def capture_gradients(optimizer):
    """-> a dict filled, at the optimizer's next zero_grad, with a copy of every gradient as the update left it."""
    seen = {}
    inner = optimizer.zero_grad

    def zero_grad(*a, **kw):
        for g in optimizer.param_groups:
            for p in g['params']:
                seen[p] = p.grad.detach().clone()
        return inner(*a, **kw)

    optimizer.zero_grad = zero_grad
    return seen


def check_first_step(optimizer, rates, before, grads, coef, eps=1e-8, tag="cpu"):
    """The first-step property of the module docstring, per parameter with its own group's rate (`rates`: what the groups
    held when the update ran); every group must hold a parameter with an element above the floor.  `grads`: the gradients
    the update used, up to the factor `coef`."""
    worst = 0.0
    for k, (group, lr) in enumerate(zip(optimizer.param_groups, rates)):
        wd, counted = group['weight_decay'], 0
        for p in group['params']:
            g = (grads[p].float() * coef).double().cpu()
            old, new = before[p].double().cpu(), p.detach().double().cpu()
            mask = g.abs() >= FLOOR
            if not bool(mask.any()):
                continue
            counted += int(mask.sum())
            top = float(old.abs().max())
            bound = eps / FLOOR + wd * top + 2.0 * ulp32(top) / lr + 8 * 2.0 ** -24
            dev = float((((new - old).abs() / lr) - 1.0).abs()[mask].max())
            worst = max(worst, dev / bound)
            assert dev <= bound, (tag, p.param_name, k, lr, dev, bound)
        assert counted > 0, f"{tag}: group {k} (lr_scale {group.get('lr_scale')}) has no gradient element above {FLOOR}"
    print(f"\n[tinyvit finetune {tag}] first step: worst deviation / bound {worst:.3f}", end="")


# ---- 14, 15: groups and schedule against the fixture ----------------------------------------------------------------------
def test_groups_against_the_fixture():
    from cream_amd import tinyvit_finetune as FT
    fix = fixture()
    model = build()
    groups = FT.finetune_param_groups(model)
    assert len(groups) == len(fix['groups']) == 10
    for g, f in zip(groups, fix['groups']):
        assert [p.param_name for p in g['params']] == f['params']
        assert ('weight_decay' in g) == (f['weight_decay'] is not None)
        if 'weight_decay' in g:
            assert g['weight_decay'] == f['weight_decay']
        assert g['lr_scale'] == f['lr_scale']
        assert set(g) == {'params', 'lr_scale'} | ({'weight_decay'} if f['weight_decay'] is not None else set())
    opt = FT.build_finetune_optimizer(model, BASE_LR, weight_decay=WEIGHT_DECAY)
    assert type(opt) is torch.optim.AdamW
    assert [g['weight_decay'] for g in opt.param_groups] == [f['weight_decay_in_optimizer'] for f in fix['groups']]
    assert [g['lr'] for g in opt.param_groups] == fix['lr_at_construction']


def test_schedule_against_the_fixture():
    from cream_amd import tinyvit_finetune as FT
    fix = fixture()
    model = build()
    opt = FT.build_finetune_optimizer(model, BASE_LR, weight_decay=WEIGHT_DECAY)
    sched = FT.LRSchedulerWrapper(WarmupCosine(opt, BASE_LR), opt)
    lrs = lambda: [g['lr'] for g in opt.param_groups]                    # noqa: E731
    assert lrs() == fix['lr_before_any_call'] and len(set(lrs())) == 1       # the inner scheduler's unscaled warm-up rate
    for it in UPDATES:
        sched.step_update(it)
        assert lrs() == fix[f'lr_after_step_update_{it}'], it
    assert len(set(lrs())) == 5
    sched.step(0)                                                            # the stand-in's step writes nothing: scaled once more
    assert lrs() == [lr * g['lr_scale'] for lr, g in zip(fix['lr_after_step_update_7'], opt.param_groups)]
    # a scale changed at run time is picked up by the next update_lr
    for p in opt.param_groups[3]['params']:
        p.lr_scale = 0.25
    sched.step_update(1)
    inner = WarmupCosine.lr_at(sched.lr_scheduler, 1)
    assert opt.param_groups[3]['lr_scale'] == 0.25 and opt.param_groups[3]['lr'] == inner * 0.25
    assert opt.param_groups[2]['lr'] == fix['lr_after_step_update_1'][2]
    assert sched.state_dict() == {'last': 1}
    sched.load_state_dict({'last': 5})
    assert sched.lr_scheduler.last == 5
    sched.step_frac(0.5)                                                     # the stand-in has no step_frac: nothing happens
    assert opt.param_groups[2]['lr'] == fix['lr_after_step_update_1'][2]


# ---- 16: the step on the CPU ----------------------------------------------------------------------------------------------
def test_finetune_step_on_the_cpu_keeps_batchnorm_and_moves_every_group_by_its_rate():
    from cream_amd import tinyvit_finetune as FT
    model = build()
    opt = FT.build_finetune_optimizer(model, STEP_LR, weight_decay=WEIGHT_DECAY)
    assert type(opt) is torch.optim.AdamW
    sched = FT.LRSchedulerWrapper(WarmupCosine(opt, STEP_LR), opt)
    sched.step_update(4)                                                     # end of warm-up: STEP_LR x lr_scale
    rates = [g['lr'] for g in opt.param_groups]
    assert rates == [STEP_LR * g['lr_scale'] for g in opt.param_groups] and len(set(rates)) == 5
    stats = bn_state(model)
    before = {p: p.detach().clone() for p in model.parameters()}
    grads = capture_gradients(opt)
    x, y = batch("cpu")
    out = FT.finetune_step(model, opt, x, y, max_norm=5.0, index=0, lr_scheduler=sched)
    assert math.isfinite(out['loss']) and out['grad_norm'] is not None and float(out['grad_norm']) > 0
    assert 0.0 <= out['acc1'] <= out['acc5'] <= 100.0
    now = bn_state(model)
    assert stats and all(torch.equal(now[k], v) for k, v in stats.items())
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert bns and not any(m.training for m in bns)
    assert all(m.training for m in model.modules() if not isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
    assert all(p.grad is None for p in model.parameters())                  # zeroed after the update (torch's default: None)
    assert sched.lr_scheduler.last == 0                                      # step_update(index // accumulation_steps) ran
    # (clip_grad_norm_ scaled the captured gradients in place: they are what the update used)
    check_first_step(opt, rates, before, grads, 1.0, tag="cpu torch.optim.AdamW")
    FT.set_bn_state(model.train(), eval_bn=False)
    assert all(m.training for m in bns)


def test_accumulation_on_the_cpu_updates_on_the_last_call_only():
    from cream_amd import tinyvit_finetune as FT
    model = build()
    opt = FT.build_finetune_optimizer(model, STEP_LR, weight_decay=WEIGHT_DECAY)
    before = [p.detach().clone() for p in model.parameters()]
    x, y = batch("cpu")
    out = FT.finetune_step(model, opt, x, y, accumulation_steps=2, index=0)
    assert out['grad_norm'] is None and all(torch.equal(p, b) for p, b in zip(model.parameters(), before))
    kept = [p.grad.clone() for p in model.parameters()]
    assert all(float(g.abs().max()) >= 0 for g in kept)
    out = FT.finetune_step(model, opt, x, y, accumulation_steps=2, index=1)
    assert out['grad_norm'] is not None and any(not torch.equal(p, b) for p, b in zip(model.parameters(), before))


# ---- 17: argument checks without a device -----------------------------------------------------------------------------------
def test_grouped_entry_point_validates_arguments_without_launching():
    from cream_amd import _lib
    lib = _lib.load()
    f = lib.cream_adamw_step_groups
    lr = (ctypes.c_double * 65)(*([1e-3] * 65))
    lrp = ctypes.cast(lr, ctypes.c_void_p)
    T, G = 0x1000, 0x2000                                                    # any non-null pointers: only checked, never read
    assert _lib.ADAMW_MAX_GROUPS == 64
    assert f(None, None, 0, 0, 1, None, lrp, 1, 0.9, 0.999, 1e-8, 1, None, None) == 0          # nothing to do
    assert f(T, T, 2, 0, 1, G, lrp, 3, 0.9, 0.999, 1e-8, 1, None, None) == 0                   # no tiles
    assert f(T, T, 2, 5, 1, G, lrp, 0, 0.9, 0.999, 1e-8, 1, None, None) == -1                  # ngroups < 1
    assert f(T, T, 2, 5, 1, G, lrp, 65, 0.9, 0.999, 1e-8, 1, None, None) == -1                 # ngroups > 64
    assert f(T, T, 2, 5, 1, G, None, 2, 0.9, 0.999, 1e-8, 1, None, None) == -1                 # no rates
    assert f(None, None, 0, 0, 1, None, None, 2, 0.9, 0.999, 1e-8, 1, None, None) == -1        # ... even with nothing to do
    assert f(T, T, 2, 5, 1, None, lrp, 2, 0.9, 0.999, 1e-8, 1, None, None) == -1               # no job -> group table
    assert f(T, T, 2, 5, 1, G, lrp, 2, 0.9, 0.999, 1e-8, 0, None, None) == -1                  # update needs step >= 1
    assert f(None, None, 2, 5, 1, G, lrp, 2, 0.9, 0.999, 1e-8, 1, None, None) == -1            # no job table
    assert f(T, T, -1, 5, 1, G, lrp, 2, 0.9, 0.999, 1e-8, 1, None, None) == -1
