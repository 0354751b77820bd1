"""TinyCLIP's mask learning on the device: the masked tower node (cream_amd/tinyclip/native_masked.py) against the fp32
composed masked mirror on the toy towers of tests/golden/make_tinyclip_l0_golden.py (image, and causal text), and five
DistillSteps with both l0 modules followed by fuse_masks."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_tinyclip_l0_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REGIONS = {"ln_fwd_masked", "ln_bwd_masked", "mask_pack", "mask_grad_finalize"}


def _run(model, tower, native_on, amp, with_masks=True):
    """One forward / backward of a tower's encoder in training mode under the fixture's seed (the same hard-concrete draws in
    every call).  -> dict of the compared groups + the tensors of the exact assertions."""
    import cream_amd.tinyclip.model as M
    images, texts, gi, gt = (t.to(DEV) for t in G.inputs())
    enc = model._image_encoder if tower == "image" else model._text_encoder
    tr = enc.visual.transformer if tower == "image" else enc.transformer
    l0 = enc.l0_module
    if not with_masks:
        enc.l0_module = None
    M.NATIVE_TOWERS = native_on
    model.zero_grad(set_to_none=True)
    seen = {}
    hook = tr.register_forward_hook(lambda mod, args, out: seen.__setitem__("tower_out", out.detach().float()))
    try:
        torch.manual_seed(G.SEED)
        x = images.clone().requires_grad_() if tower == "image" else texts
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            f = enc(x, normalized=True)
        masks = dict(enc.mask)
        for v in masks.values():
            v.retain_grad()
        (f.float() * (gi if tower == "image" else gt)).sum().backward()
        torch.cuda.synchronize()
    finally:
        hook.remove()
        enc.l0_module = l0
        M.NATIVE_TOWERS = True
    out = dict(output=f.detach().float(), tower_out=seen["tower_out"],
               input_grad=x.grad.clone() if tower == "image" else enc.positional_embedding.grad.clone(),
               weights={k: p.grad.clone() for k, p in tr.named_parameters()}, masks={k: v.detach() for k, v in masks.items()})
    if with_masks:
        out.update({k: v.grad.clone() for k, v in masks.items()})
        out["loga"] = {k: p.grad.clone() for k, p in l0.named_parameters() if "loga" in k}
    return out


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("tower", ["image", "text"])
def test_masked_native_tower_matches_the_composed_mirror(tower):
    """Native masked under bf16 autocast and — measured in the same test — the composed masked mirror under bf16 autocast,
    both against the fp32 composed masked mirror; the project's form (tests/test_tinyclip_model.py:174-175) per group."""
    from cream_amd import timing
    from cream_amd.tinyclip.model import CLIP
    model = G.build(CLIP).to(DEV)
    ref = _run(model, tower, False, False)
    timing.reset()
    timing.enable(True)
    nat = _run(model, tower, True, True)
    timing.enable(False)
    assert REGIONS <= set(timing.summary()), set(timing.summary())
    timing.reset()
    timing.enable(True)
    dense = _run(model, tower, True, True, with_masks=False)
    timing.enable(False)
    s = set(timing.summary())
    timing.reset()
    assert "ln_fwd" in s and not (REGIONS & s), s                      # a call without masks: the dense node, none of the new launches
    mod = _run(model, tower, False, True)
    for k in ("hidden_z", "heads_z", "intermediate_z"):                # the same draws in every run, with exact zeros
        assert torch.equal(nat["masks"][k], ref["masks"][k]) and torch.equal(mod["masks"][k], ref["masks"][k])
        assert bool((ref["masks"][k] == 0).any())

    def groups(r):
        g = {"output": _rel(r["output"], ref["output"]), "input gradient": _rel(r["input_grad"], ref["input_grad"]),
             "weight gradients": max(_rel(r["weights"][k], ref["weights"][k]) for k in ref["weights"]),
             "log-alpha gradients": max(_rel(r["loga"][k], ref["loga"][k]) for k in ref["loga"])}
        g.update({f"d {k}": _rel(r[k], ref[k]) for k in ("hidden_z", "heads_z", "intermediate_z")})
        return g
    e_nat, e_mod = groups(nat), groups(mod)
    for k in e_nat:
        print(f"[tinyclip l0 {tower}] {k}: native bf16 {e_nat[k]:.2e}, composed bf16 autocast {e_mod[k]:.2e} (both vs fp32 composed)")
    for k in e_nat:
        assert e_nat[k] < 1.5 * e_mod[k] + 5e-3 and e_nat[k] < 3e-2, (k, e_nat[k], e_mod[k])

    zh = ref["masks"]["hidden_z"]
    zd = ref["masks"]["heads_z"].reshape(2, 2)
    zi = ref["masks"]["intermediate_z"].reshape(2, -1)
    assert bool((nat["tower_out"][..., zh == 0] == 0).all())
    for i in range(2):
        wo, w2 = nat["weights"][f"resblocks.{i}.attn.out_proj.weight"], nat["weights"][f"resblocks.{i}.mlp.c_proj.weight"]
        assert bool((wo[zh == 0] == 0).all()) and bool((w2[zh == 0] == 0).all())
        assert bool((wo[:, zd[i].repeat_interleave(64) == 0] == 0).all()) and bool((w2[:, zi[i] == 0] == 0).all())
        assert bool((nat["weights"][f"resblocks.{i}.attn.out_proj.bias"][zh == 0] == 0).all())
        for ln in ("ln_1", "ln_2"):
            for wb in ("weight", "bias"):
                assert bool((nat["weights"][f"resblocks.{i}.{ln}.{wb}"][zh == 0] == 0).all()), (i, ln, wb)


def test_masked_native_tower_without_mask_gradients():
    """eval / no_grad: the deterministic masks, nothing saved, the same features as the composed path; the operand pack is
    reused across forwards while the l0 parameters keep their versions."""
    import cream_amd.tinyclip.model as M
    from cream_amd import timing
    from cream_amd.tinyclip.model import CLIP
    model = G.build(CLIP).to(DEV).eval()
    images = G.inputs()[0].to(DEV)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            M.NATIVE_TOWERS = False
            f_mod = model.encode_image(images, normalized=True).float()
            M.NATIVE_TOWERS = True
            timing.reset()
            timing.enable(True)
            f_nat = model.encode_image(images, normalized=True).float()
            f_again = model.encode_image(images, normalized=True).float()
            timing.enable(False)
    finally:
        M.NATIVE_TOWERS = True
    s = timing.summary()
    timing.reset()
    assert s["ln_fwd_masked"]["launches"] == 8 and s["mask_pack"]["launches"] == 2, s          # 2 blocks packed once, 2 x 2 x 2 LayerNorms
    assert torch.equal(f_nat, f_again) and _rel(f_nat, f_mod) < 3e-2


def test_distill_steps_learn_masks_and_fuse():
    """Five steps per Lagrangian mode under bf16 autocast (the masked native node in the loop), then fuse_masks on 0 / 1
    masks: the pruned student (composed, bf16 autocast) against its own masked eval features (native) — two bf16 evaluations
    of one function, held to the project's bf16 bound of 3e-2."""
    from cream_amd import timing
    from test_tinyclip_l0_cpu import mask_learning_run
    timing.reset()
    timing.enable(True, only=REGIONS)
    try:
        err = mask_learning_run(DEV, torch.bfloat16)
    finally:
        timing.enable(False)
    s = timing.summary()
    timing.reset()
    assert REGIONS <= set(s), set(s)
    print(f"[tinyclip l0 fuse] pruned vs masked eval features {err:.2e}")
    assert err < 3e-2
