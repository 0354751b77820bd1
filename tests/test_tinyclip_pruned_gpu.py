"""Pruned TinyCLIP towers on the device: the node of cream_amd/tinyclip/native_pruned.py on the toy tower of
tests/pruned_ref.py (hand-set 0 / 1 masks, prune()) against the fp32 composed pruned tower, its lost branches, and two
DistillSteps on the fused toy student of tests/golden/make_tinyclip_l0_golden.py."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pruned_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REGIONS = {"gemm_nt", "ln_fwd_masked", "grad_finalize_compact"}
B = 3


def _run(tr, x0, g, causal, native_on, amp):
    """One forward / backward of the tower.  -> (output, input gradient, {name: parameter gradient}, regions seen)"""
    import cream_amd.tinyclip.model as M
    from cream_amd import timing
    L = x0.shape[1]
    mask = torch.full((L, L), float("-inf"), device=DEV).triu_(1) if causal else None
    tr.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_()
    M.NATIVE_TOWERS = native_on
    timing.reset()
    timing.enable(True)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out = tr(x, attn_mask=mask, causal=causal)
        (out.float() * g).sum().backward()
        seen = set(timing.summary())
    finally:
        timing.enable(False)
        timing.reset()
        M.NATIVE_TOWERS = True
    return out.detach().float(), x.grad.clone(), {k: p.grad.clone() for k, p in tr.named_parameters()}, seen


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def towers():
    cache = {}

    def get(keep):
        if keep not in cache:
            cache[keep] = R.toy_tower(keep).to(DEV)
        return cache[keep]
    return get


@pytest.mark.parametrize("keep", [101, 96, 9])
@pytest.mark.parametrize("causal,L", [(False, 37), (True, 13)])
def test_pruned_native_tower_matches_the_composed_tower(towers, keep, causal, L):
    """Native pruned under bf16 autocast and — in the same test — composed pruned under bf16 autocast, both against the fp32
    composed pruned tower; the project's form (tests/test_tinyclip_l0_gpu.py) per group."""
    from cream_amd.tinyclip import native_pruned
    tr = towers(keep)
    pl = native_pruned.plan(tr)
    assert pl["d"] == keep and pl["Dp"] == {101: 104, 96: 96, 9: 16}[keep]
    gen = torch.Generator().manual_seed(3)
    x0 = torch.randn(B, L, keep, generator=gen).to(DEV)
    g = torch.randn(B, L, keep, generator=gen).to(DEV)
    shapes = {k: tuple(v.shape) for k, v in tr.state_dict().items()}
    ref = _run(tr, x0, g, causal, False, False)
    nat = _run(tr, x0, g, causal, True, True)
    mod = _run(tr, x0, g, causal, False, True)                                           # NATIVE_TOWERS = False: the same call, composed
    assert REGIONS <= nat[3], nat[3]
    assert not (REGIONS & mod[3]) and not (REGIONS & ref[3]), (mod[3], ref[3])
    assert {k: tuple(v.shape) for k, v in tr.state_dict().items()} == shapes             # the compact shapes, untouched
    assert set(nat[2]) == set(ref[2]) and all(nat[2][k].shape == tr.get_parameter(k).shape for k in nat[2])
    assert nat[0].shape == (B, L, keep) and nat[1].shape == (B, L, keep)

    def groups(r):
        return {"output": _rel(r[0], ref[0]), "input gradient": _rel(r[1], ref[1]),
                "parameter gradients": max(_rel(r[2][k], ref[2][k]) for k in ref[2])}
    e_nat, e_mod = groups(nat), groups(mod)
    for k in e_nat:
        print(f"[tinyclip pruned keep={keep} causal={causal}] {k}: native bf16 {e_nat[k]:.2e}, composed bf16 autocast {e_mod[k]:.2e} "
              "(both vs fp32 composed)")
    for k in e_nat:
        assert e_nat[k] < 1.5 * e_mod[k] + 5e-3 and e_nat[k] < 3e-2, (k, e_nat[k], e_mod[k])


def test_lost_branches_and_the_identity_block(towers):
    """The both-lost block is the identity, exactly; the attention-less and the MLP-less block get gradients for exactly their
    remaining parameters."""
    from cream_amd.tinyclip import native_pruned
    tr = towers(101)
    gen = torch.Generator().manual_seed(4)
    x0 = torch.randn(B, 7, 101, generator=gen).to(DEV)
    g = torch.randn(B, 7, 101, generator=gen).to(DEV)
    assert [n for n, _ in tr.resblocks[4].named_parameters()] == []
    assert {n.split(".")[0] for n, _ in tr.resblocks[2].named_parameters()} == {"ln_2", "mlp"}
    assert {n.split(".")[0] for n, _ in tr.resblocks[3].named_parameters()} == {"ln_1", "attn"}
    full = _run(tr, x0, g, False, True, True)
    assert "grad_finalize_compact" in full[3]
    assert all(v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in full[2].values())
    assert len(full[2]) == sum(1 for _ in tr.parameters())
    head = _run(R.sub_tower(tr, [0, 1, 2, 3]), x0, g, False, True, True)
    assert torch.equal(full[0], head[0]) and torch.equal(full[1], head[1])               # block 4 changes nothing, bit for bit
    assert all(torch.equal(full[2][k], head[2][k]) for k in head[2])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        only = R.sub_tower(tr, [4])
        assert native_pruned.supported(only, x0, None)
        y = only(x0)
    assert torch.equal(y, x0)
    for idx in ([2], [3], [3, 4, 2]):                                                    # single halves and a chain across a missing half
        sub = R.sub_tower(tr, idx)
        ref = _run(sub, x0, g, False, False, False)
        nat = _run(sub, x0, g, False, True, True)
        assert REGIONS <= nat[3] and set(nat[2]) == set(ref[2])
        errs = [_rel(nat[0], ref[0]), _rel(nat[1], ref[1])] + [_rel(nat[2][k], ref[2][k]) for k in ref[2]]
        print(f"[tinyclip pruned blocks {idx}] worst {max(errs):.2e}")
        assert max(errs) < 3e-2, (idx, errs)


def _mirrors_padding_is_zero(student):
    from cream_amd.tinyclip import native_pruned
    n = 0
    for enc_tr in (student._image_encoder.visual.transformer, student._text_encoder.transformer):
        for blk in enc_tr.resblocks:
            ops = blk.__dict__.get(native_pruned._OPS_KEY)
            if ops is None:
                continue
            for (w, b, _, _), mw, mwt, mb in zip(ops.pairs, ops.w, ops.wt, ops.b):
                r, c = w.shape
                assert bool((mw[r:] == 0).all()) and bool((mw[:, c:] == 0).all()) and bool((mwt[c:] == 0).all()) and bool((mwt[:, r:] == 0).all())
                assert bool((mb[r:] == 0).all())
                assert torch.equal(mw[:r, :c], w.detach().to(torch.bfloat16)) and torch.equal(mwt[:c, :r], w.detach().t().to(torch.bfloat16))
                n += 1
            for ln, (gm, bt) in zip(ops.lns, ops.ln):
                d = ln.weight.shape[0]
                assert bool((gm[d:] == 0).all()) and bool((bt[d:] == 0).all()) and torch.equal(gm[:d], ln.weight.detach())
    return n


def test_distill_steps_on_the_fused_student(monkeypatch):
    import make_tinyclip_l0_golden as G
    from test_tinyclip_l0_cpu import _binary_masks
    from cream_amd import timing
    from cream_amd.autoformer import block as K
    from cream_amd.tinyclip import distill, native_pruned
    from cream_amd.tinyclip.model import CLIP
    student = G.build(CLIP)
    _binary_masks(student)
    G.fuse(student)
    torch.manual_seed(3)
    teacher = CLIP(32, vision_cfg=dict(G.CASE["vision_cfg"]), text_cfg=dict(G.CASE["text_cfg"]))
    student, teacher = student.to(DEV), teacher.to(DEV)
    tri = student._image_encoder.visual.transformer
    assert native_pruned.plan(tri)["d"] < 128
    images, texts = (t.to(DEV) for t in G.inputs()[:2])
    opt = torch.optim.AdamW(distill.student_parameters(student), lr=1e-3)
    step = distill.DistillStep(student, teacher, opt)

    def features():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return student(images, texts, normalized=True)
    student.eval()
    wants = []
    real = K.linear_gelu_fwd
    monkeypatch.setattr(K, "linear_gelu_fwd", lambda *a, **k: (wants.append(k.get("want_grad", True)), real(*a, **k))[1])
    timing.reset()
    timing.enable(True, only=REGIONS)
    try:
        f0 = features()
        f0b = features()
        seen = set(timing.summary())
    finally:
        timing.enable(False)
        timing.reset()
    assert REGIONS - {"grad_finalize_compact"} <= seen and "grad_finalize_compact" not in seen
    assert wants and not any(wants)                                                      # no_grad: nothing kept for a backward
    assert all(t.grad_fn is None for t in f0[:2]) and torch.equal(f0[0], f0b[0]) and torch.equal(f0[1], f0b[1])
    assert _mirrors_padding_is_zero(student) > 0
    student.train()
    losses = [float(step.step(images, texts)) for _ in range(2)]
    assert all(math.isfinite(v) for v in losses), losses
    assert all(p.grad is not None and p.grad.shape == p.shape for p in distill.student_parameters(student))
    student.eval()
    f1 = features()
    assert not torch.equal(f1[0], f0[0]) and not torch.equal(f1[1], f0[1])                # the operands were refreshed after the steps
    assert bool(torch.isfinite(f1[0]).all()) and bool(torch.isfinite(f1[1]).all())
    assert _mirrors_padding_is_zero(student) > 0
