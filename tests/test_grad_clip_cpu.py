"""Global-norm gradient clipping without a device: the float64 reference of tests/clip_ref.py against the framework, the C ABI
of the three new entry points (declared, exported, argument checks that return before any launch), the framework path of
cream_amd.grad_clip and the CPU behaviour of SupernetTrainer(max_norm=...)."""
import math
import os
import random
import re

import pytest
import torch

import clip_ref
from conftest import ROOT

NEW = ("cream_grad_clip_coef", "cream_adamw_step_clipped", "cream_grad_scale")


def _grads(scale, dtype=torch.float64):
    g = torch.Generator().manual_seed(5)
    return [torch.randn(s, generator=g, dtype=torch.float64).mul(scale).to(dtype) for s in ((1,), (37,), (5, 3), (97, 65), (2, 3, 130))]


@pytest.mark.parametrize("case", ["above", "below", "zero", "inf"])
def test_clip_ref_is_the_framework_function_in_float64(case):
    grads = _grads(0.0 if case == "zero" else 1.0)
    norm64 = math.sqrt(sum(float((g * g).sum()) for g in grads))
    max_norm = {"above": 0.25 * norm64, "below": 4.0 * norm64, "zero": 1.0, "inf": math.inf}[case]
    params = [torch.nn.Parameter(g.clone()) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    fw_norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    norm, coef, scaled = clip_ref.clip(grads, max_norm)
    assert abs(norm - float(fw_norm)) <= 4 * 2.0 ** -52 * norm
    assert (coef < 1.0) == (case == "above")
    if case == "zero":
        assert norm == 0.0 and coef == 1.0
    for p, s in zip(params, scaled):
        assert torch.allclose(p.grad, s, rtol=8 * 2.0 ** -52, atol=0.0)
    if case == "above":                                              # the clipped gradients have norm max_norm
        assert abs(clip_ref.clip(scaled, math.inf)[0] - max_norm) <= 1e-6 * max_norm


def test_new_symbols_in_header_library_and_table():
    import ctypes
    from cream_amd import _lib
    text = open(os.path.join(ROOT, "include", "cream_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    # cream_adamw_step_clipped = the arguments of cream_adamw_step, the coefficient, the stream
    a, b = _lib.SIGNATURES["cream_adamw_step"][1], _lib.SIGNATURES["cream_adamw_step_clipped"][1]
    assert b[:-2] == a[:-1] and len(b) == len(a) + 1


def test_clip_entry_points_validate_arguments_without_launching():
    from cream_amd import _lib
    lib = _lib.load()
    P = 0x1000                                                       # any non-null pointer: only checked, never read
    inf, nan = math.inf, math.nan
    coef = lib.cream_grad_clip_coef
    assert coef(P, P, -1, 5, 1.0, P, P, None) == -1                  # negative counts
    assert coef(P, P, 2, -1, 1.0, P, P, None) == -1
    assert coef(P, P, 2, 5, 1.0, P, None, None) == -1                # NULL out
    assert coef(None, P, 2, 5, 1.0, P, P, None) == -1                # NULL tables with njobs > 0
    assert coef(P, None, 2, 5, 1.0, P, P, None) == -1
    assert coef(P, P, 2, 5, 1.0, None, P, None) == -1                # NULL workspace with tiles to reduce
    for bad in (0.0, -1.0, -inf, nan):
        assert coef(P, P, 2, 5, bad, P, P, None) == -1
        assert coef(None, None, 0, 0, bad, None, P, None) == -1
    step = lib.cream_adamw_step_clipped
    args = (1, 1e-3, 0.9, 0.999, 1e-8)
    assert step(P, P, -1, 5, *args, 1, P, None) == -1
    assert step(P, P, 2, -5, *args, 1, P, None) == -1
    assert step(P, P, 2, 5, *args, 1, None, None) == -1              # NULL coefficient
    assert step(None, None, 0, 0, *args, 1, None, None) == -1
    assert step(None, None, 2, 5, *args, 1, P, None) == -1           # NULL tables
    assert step(P, P, 2, 5, *args, 0, P, None) == -1                 # update needs step >= 1
    assert step(None, None, 0, 0, *args, 1, P, None) == 0            # nothing to do
    assert step(None, None, 0, 0, 0, 1e-3, 0.9, 0.999, 1e-8, 0, P, None) == 0    # copy mode: no step number needed
    scale = lib.cream_grad_scale
    assert scale(None, None, 0, 0, P, None) == 0                     # nothing to do
    assert scale(P, P, 0, 7, P, None) == 0
    assert scale(P, P, -1, 0, P, None) == -1
    assert scale(P, P, 1, -1, P, None) == -1
    assert scale(P, P, 1, 1, None, None) == -1                       # NULL coefficient
    assert scale(None, None, 0, 0, None, None) == -1
    assert scale(None, P, 1, 1, P, None) == -1                       # NULL tables
    assert scale(P, None, 1, 1, P, None) == -1
    # cream_adamw_step itself is as it was
    assert lib.cream_adamw_step(None, None, 0, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None) == 0
    assert lib.cream_adamw_step(None, None, 2, 5, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None) == -1


def _params_with(grads):
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=g.dtype)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    return ps


@pytest.mark.parametrize("case", ["fp32", "one_bf16", "one_none", "single_tensor"])
def test_grad_clip_on_cpu_tensors_is_the_framework_function(case):
    from cream_amd import grad_clip
    grads = _grads(1.0, torch.float32)
    if case == "one_bf16":
        grads[2] = grads[2].bfloat16()
    for max_norm in (0.5, 1e4):
        a, b = _params_with(grads), _params_with(grads)
        if case == "one_none":
            a[1].grad = b[1].grad = None
        if case == "single_tensor":
            a, b = a[3], b[3]
        na = grad_clip.clip_grad_norm_(a, max_norm)
        nb = torch.nn.utils.clip_grad_norm_(b, max_norm)
        assert torch.equal(na, nb) and na.dtype == nb.dtype
        a, b = ([a], [b]) if case == "single_tensor" else (a, b)
        for p, q in zip(a, b):
            assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad)


def test_supernet_trainer_with_max_norm_on_the_cpu_clips_then_steps():
    """SupernetTrainer(max_norm=1.0) on the CPU: build_optimizer gives torch.optim.AdamW, and the parameters after one step
    equal a hand-written clip + step on a twin model."""
    from cream_amd.autoformer import engine
    torch.manual_seed(0)
    kw = dict(depth=2, drop_path_rate=0.0, num_classes=10, img_size=32)
    m, twin = engine.build_supernet("T", **kw), engine.build_supernet("T", **kw)
    twin.load_state_dict(m.state_dict())
    opt, opt_t = engine.build_optimizer(m, batch_size=4), engine.build_optimizer(twin, batch_size=4)
    assert type(opt) is torch.optim.AdamW
    choices = dict(mlp_ratio=[3.5, 4], num_heads=[3, 4], depth=[2], embed_dim=[192, 216])
    tr = engine.SupernetTrainer(m, opt, choices, amp_dtype=torch.float32, max_norm=1.0)
    images = torch.randn(4, 3, 32, 32)
    target = torch.softmax(torch.randn(4, 10), dim=-1)
    tr.start_epoch(3)
    loss = tr.step(images, target)
    # the twin: same draw, same forward / backward, then clip and step written out
    random.seed(3)
    twin.train()
    twin.set_sample_config(engine.sample_configs(choices))
    opt_t.zero_grad(set_to_none=False)
    loss_t = engine.soft_target_cross_entropy(twin(images), target)
    loss_t.backward()
    grads = [p.grad for p in twin.parameters() if p.grad is not None]
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    assert float(norm) > 1.0, "the case must clip"
    c = torch.clamp(1.0 / (norm + 1e-6), max=1.0)
    for g in grads:
        g.mul_(c)
    opt_t.step()
    assert torch.equal(loss, loss_t)
    for (n, p), q in zip(m.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), n
