"""Fused Mini-DeiT attention with head transforms (cream_amd/mini_attn.py, csrc/mini_attn.hip) on the GPU:
A. the kernels against the module's own composed branch (fp32 reference, bf16 composed as the yardstick of bf16 noise),
B. the registered mini_deit('tiny') against the upstream-made fixture, on the fused path,
C. the repeat counter selects tables and convolutions on the fused path,
D. bit-identical reruns,
E. what the kernels do not cover falls back to the composed branch."""
import os
from contextlib import contextmanager

import pytest
import torch

from helpers import max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = {"mini_attn_fwd", "mini_attn_bwd"}


@contextmanager
def fused_off():
    old = os.environ.get("CREAM_IRPE_FUSED")
    os.environ["CREAM_IRPE_FUSED"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CREAM_IRPE_FUSED"]
        else:
            os.environ["CREAM_IRPE_FUSED"] = old


def make_attn(H, shared=True, skip=0, rpe_on='k', attn_drop=0.0, seed=0):
    from cream_amd import minivit
    from cream_amd.irpe import get_rpe_config
    cfg = None
    if rpe_on:
        cfg = get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=shared, skip=skip, rpe_on=rpe_on)
    torch.manual_seed(seed)
    m = minivit.MiniAttention(H * 64, num_heads=H, qkv_bias=True, rpe_config=cfg, repeated_times=1, use_transform=True,
                              attn_drop=attn_drop)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'lookup_table' in n:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif 'conv_' in n:      # eye + 0.3 randn: non-symmetric, so [o,h] / [h,o] or swapped convolutions show
                p.copy_((torch.eye(H) + 0.3 * torch.randn(H, H, generator=g)).reshape(H, H, 1, 1))
    return m.to(DEV)


def tensors_of(m):
    out = {"d qkv.weight": m.qkv.weight.grad, "d conv_l": m.conv_l.instances[0].weight.grad,
           "d conv_w": m.conv_w.instances[0].weight.grad}
    if m.rpe_k is not None:
        out["d table"] = m.rpe_k.instances[0].lookup_table_weight.grad
    return out


def run_attn(m, x, gy, autocast, fused):
    """-> ({name: tensor}, regions seen)"""
    from cream_amd import timing
    m.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    timing.reset()
    timing.enable(True)
    try:
        if fused:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = m(x)
        else:
            with fused_off(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = m(x)
        (y.float() * gy).sum().backward()
    finally:
        timing.enable(False)
    res = {"out": y.detach().float().cpu(), "dx": x.grad.detach().float().cpu()}
    res.update({k: v.detach().float().cpu() for k, v in tensors_of(m).items()})
    return res, set(timing.summary())


CASES = {
    "H3_L196_shared": dict(H=3, L=196, B=2),
    # one full and one partial tile, per-head table.  The module's composed branch (the reference) takes L as a square grid plus
    # L - floor(sqrt(L))^2 leading tokens that share the skip bucket, so L = 40 = 4 + 6 x 6 needs a skip = 1 table (50 buckets)
    "H6_L40_perhead": dict(H=6, L=40, B=2, shared=False, skip=1),
    "H6_L36_perhead_skip0": dict(H=6, L=36, B=2, shared=False),
    "H12_L196_shared": dict(H=12, L=196, B=2),
    "H12_L576": dict(H=12, L=576, B=1),
    "H3_L197_cls_skip1": dict(H=3, L=197, B=2, skip=1),
    "H2_L64_norpe": dict(H=2, L=64, B=2, rpe_on=''),
}


def case_inputs(c, seed=5):
    g = torch.Generator().manual_seed(seed)
    E = c["H"] * 64
    x = torch.randn(c["B"], c["L"], E, generator=g).bfloat16().float().to(DEV)          # the same bf16-rounded input for all
    gy = torch.randn(c["B"], c["L"], E, generator=g).to(DEV)
    return x, gy


@pytest.mark.parametrize("tag", list(CASES))
def test_fused_against_composed(tag):
    """err(fused) <= max(2 err(composed bf16), 2^-7) for every tensor, both against the fp32 composed branch."""
    c = CASES[tag]
    m = make_attn(c["H"], shared=c.get("shared", True), skip=c.get("skip", 0), rpe_on=c.get("rpe_on", 'k'))
    x, gy = case_inputs(c)
    ref, names_a = run_attn(m, x, gy, autocast=False, fused=True)        # fp32: the module itself stays composed
    comp, names_b = run_attn(m, x, gy, autocast=True, fused=False)
    fus, names_c = run_attn(m, x, gy, autocast=True, fused=True)
    assert not NEW & names_a and not NEW & names_b, (names_a, names_b)
    assert NEW <= names_c, names_c
    bad = []
    for k in ref:
        eb, ec = max_rel(comp[k], ref[k]), max_rel(fus[k], ref[k])
        bound = max(2 * eb, 2.0 ** -7)
        print(f"[mini_attn {tag}] {k:14s} composed bf16 {eb:.3e}  fused {ec:.3e}  bound {bound:.3e}")
        if not ec <= bound:
            bad.append((k, eb, ec))
    assert not bad, bad


def test_whole_model_on_fixture_takes_the_fused_path():
    from test_minivit import build, compare, run
    from cream_amd import timing
    tag = "mini_deit_tiny"
    model = build(tag).to(DEV)
    timing.reset()
    timing.enable(True)
    logits, grads = run(model, tag, DEV, autocast=True)
    timing.enable(False)
    names = set(timing.summary())
    assert NEW <= names and not {"rpe_index_fwd", "rpe_index_bwd"} & names, names
    worst = compare(tag, logits, grads, 4e-2)
    print(f"[minivit gpu bf16 mixed {tag}] worst {worst:.2e}")


def test_repeat_counter_selects_the_instances_on_the_fused_path():
    from cream_amd import minivit, timing
    from cream_amd.irpe import get_rpe_config
    cfg = get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=True, skip=0, rpe_on='k')
    torch.manual_seed(1)
    blk = minivit.RepeatedMiniBlock(repeated_times=2, dim=128, num_heads=2, qkv_bias=True, rpe_config=cfg, drop_paths=[0., 0.],
                                    use_transform=True).eval()
    with torch.no_grad():
        for m in blk.block.attn.rpe_k.instances:
            m.lookup_table_weight.normal_(std=0.3)
        for convs in (blk.block.attn.conv_l, blk.block.attn.conv_w):
            for c in convs.instances:
                c.weight.copy_((torch.eye(2) + 0.3 * torch.randn(2, 2)).reshape(2, 2, 1, 1))
    blk = blk.to(DEV)
    x = torch.randn(1, 16, 128, device=DEV)
    timing.reset()
    timing.enable(True)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = blk(x)
        blk._set_repeat(0)
        y0 = blk.block(x)
        blk.block.attn.rpe_k.instances[1].lookup_table_weight.zero_()
        y1 = blk(x)
        assert not torch.equal(y1, y)
        blk._set_repeat(0)
        assert torch.equal(blk.block(x), y0)
        blk.block.attn.conv_w.instances[1].weight.zero_()
        assert not torch.equal(blk(x), y1)
        blk._set_repeat(0)
        assert torch.equal(blk.block(x), y0)
    timing.enable(False)
    names = set(timing.summary())
    assert "mini_attn_fwd" in names and "rpe_index_fwd" not in names, names


def test_reruns_are_bit_identical():
    c = CASES["H12_L196_shared"]
    m = make_attn(c["H"])
    x, gy = case_inputs(c)
    a, names = run_attn(m, x, gy, autocast=True, fused=True)
    b, _ = run_attn(m, x, gy, autocast=True, fused=True)
    assert NEW <= names
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("what", ["dropout_training", "rpe_qk", "fp32"])
def test_uncovered_configurations_stay_composed(what):
    H, L, B = 2, 64, 2
    m = make_attn(H, rpe_on='qk' if what == "rpe_qk" else 'k', attn_drop=0.1 if what == "dropout_training" else 0.0)
    m.train(what == "dropout_training")
    x, gy = case_inputs(dict(H=H, L=L, B=B))
    autocast = what != "fp32"
    torch.manual_seed(11)
    a, names = run_attn(m, x, gy, autocast=autocast, fused=True)
    assert not NEW & names, names
    torch.manual_seed(11)
    b, _ = run_attn(m, x, gy, autocast=autocast, fused=False)            # the composed branch, selected by the switch
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_eval_mode_with_attn_drop_takes_the_fused_path():
    m = make_attn(2, attn_drop=0.1).eval()
    x, gy = case_inputs(dict(H=2, L=64, B=2))
    _, names = run_attn(m, x, gy, autocast=True, fused=True)
    assert NEW <= names, names
