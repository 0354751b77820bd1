"""TinyCLIP's mask learning on the CPU: the mirror (cream_amd/tinyclip/l0.py, the mask arguments and prune() of
cream_amd/tinyclip/model.py, the mask part of cream_amd/tinyclip/distill.py) against the fixture made by the reference's own
classes (tests/golden/make_tinyclip_l0_golden.py), and the properties that need no fixture."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from helpers import load_json, load_npz, max_rel  # noqa: E402
import make_tinyclip_l0_golden as G  # noqa: E402

TOL = 2e-4          # the fp32 bound tests/test_tinyclip_model.py holds its CPU fixture to


@pytest.fixture(scope="module")
def fix():
    return load_npz("tinyclip_l0.npz"), load_json("tinyclip_l0.json")


def mirror():
    from cream_amd.tinyclip.model import CLIP
    return G.build(CLIP)


def test_state_dict_keys_are_the_references(fix):
    _, meta = fix
    model = mirror()
    assert list(model.state_dict().keys()) == meta["keys"]
    for tower, enc in (("image", model._image_encoder), ("text", model._text_encoder)):
        assert {k: list(v) for k, v in enc.l0_module.shapes.items()} == meta[tower]["shapes"]
        assert enc.l0_module.prunable_model_size == meta[tower]["prunable_model_size"]


def test_training_step_matches_the_reference(fix):
    """Masks bit for bit (same draws from the same seed); features, loss and every gradient — the l0 parameters' included —
    to the fp32 tolerance."""
    arrays, _ = fix
    model = mirror()
    fi, ft, scale, loss, masks = G.train_step(model)
    for tower, mk in zip(("image", "text"), masks):
        assert set(mk) == {"hidden_z", "heads_z", "intermediate_z"}
        for k, v in mk.items():
            ref = torch.from_numpy(arrays[f"{tower}|train|{k}"])
            assert v.shape == ref.shape and torch.equal(v.detach(), ref), (tower, k)
    errs = {"image_features": max_rel(fi.detach(), arrays["image_features"]), "text_features": max_rel(ft.detach(), arrays["text_features"]),
            "loss": abs(float(loss.detach()) - float(arrays["loss"][0])) / abs(float(arrays["loss"][0]))}
    grads = {k: p.grad for k, p in model.named_parameters()}
    for k, v in arrays.items():
        if k.startswith("grad|") and k.endswith("|norm"):
            name = k[5:-5]
            ref = float(v[0])
            g = grads[name].detach().double().flatten()
            if ref < 1e-9:
                assert float(g.norm()) < 1e-6, name
                continue
            errs[name + "|norm"] = abs(float(g.norm()) - ref) / ref
            s = ref / max(1.0, g.numel()) ** 0.5
            errs[name + "|sample"] = float((g[::G.STRIDE] - torch.from_numpy(arrays[f"grad|{name}|sample"])).abs().max() / s) / 10.0
    assert any("l0_module.hidden_loga" in k for k in errs) and any("l0_module.lambda_1" in k for k in errs)
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    print(f"[tinyclip l0 cpu] worst {max(errs.values()):.2e} over {len(errs)} records")
    assert not bad, ", ".join(f"{k}={e:.2e}" for k, e in sorted(bad.items(), key=lambda t: -t[1])[:8])


def test_host_side_quantities_match_the_reference(fix):
    arrays, meta = fix
    model = mirror()
    for tower, enc in (("image", model._image_encoder), ("text", model._text_encoder)):
        a, mt = G.l0_records(enc.l0_module)
        for k, v in a.items():
            ref = torch.from_numpy(arrays[f"{tower}|{k}"])
            v = torch.as_tensor(v)
            assert v.shape == ref.shape, (tower, k)
            if k.startswith(("eval|", "l0_mask|")):
                assert torch.equal((v == 0), (ref == 0)), (tower, k)                   # the same entries cut
            assert torch.allclose(v.double(), ref.double(), rtol=1e-6, atol=1e-7), (tower, k)
        assert mt["model_size"] == meta[tower]["model_size"], tower


def test_eval_and_pruned_models_match_the_reference(fix):
    """prune() literally as the reference: keys, shapes and — the eval masks are NOT 0/1, so pruned != masked — the pruned
    model's own features."""
    arrays, meta = fix
    model = mirror()
    images, texts, _, _ = G.inputs()
    with torch.no_grad():
        model.eval()
        fi, ft, _ = model(images, texts, normalized=True)
    assert max_rel(fi, arrays["eval|image_features"]) < TOL and max_rel(ft, arrays["eval|text_features"]) < TOL
    G.fuse(model)
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == meta["pruned"]
    with torch.no_grad():
        fi, ft, _ = model(images, texts, normalized=True)
    assert max_rel(fi, arrays["pruned|image_features"]) < TOL and max_rel(ft, arrays["pruned|text_features"]) < TOL


def _binary_masks(model):
    for enc in (model._image_encoder, model._text_encoder):
        l0 = enc.l0_module
        with torch.no_grad():
            for p in l0.z_logas.values():
                p.copy_(torch.where(p > 0, torch.full_like(p, 40.0), torch.full_like(p, -40.0)))   # sigmoid -> exactly 1 / cut to 0


def test_pruned_equals_masked_for_binary_masks():
    model = mirror()
    _binary_masks(model)
    images, texts, _, _ = G.inputs()
    with torch.no_grad():
        model.eval()
        fi0, ft0, _ = model(images, texts, normalized=True)
        for m in (model._image_encoder.mask, model._text_encoder.mask):
            for k, v in m.items():
                assert bool(((v == 0) | (v == 1)).all()) and bool((v == 0).any()), k
    n0 = sum(p.numel() for p in model.parameters())
    G.fuse(model)
    assert sum(p.numel() for p in model.parameters()) < n0
    with torch.no_grad():
        fi1, ft1, _ = model(images, texts, normalized=True)
    # fp32, the same sums over fewer (exactly zero) terms: rounding of a different summation order only
    assert max_rel(fi1, fi0) < 1e-5 and max_rel(ft1, ft0) < 1e-5, (max_rel(fi1, fi0), max_rel(ft1, ft0))


def test_native_supported_refuses_a_pruned_tower(monkeypatch):
    """Looked at through the parameter shapes: inner = 64 H_l != D, per-layer widths.  (No device here: every other condition
    is made true so that the shapes decide.)"""
    from cream_amd.tinyclip import native
    model = mirror()
    tr = model._image_encoder.visual.transformer
    x = torch.zeros(2, 5, 128)
    monkeypatch.setattr(native, "_environment_ok", lambda *a, **k: True)
    assert native.supported(tr, x, None) is True
    _binary_masks(model)
    G.fuse(model)
    tr = model._image_encoder.visual.transformer
    assert tr.resblocks[0].attn.in_proj_weight.shape[0] != 3 * tr.resblocks[0].attn.in_proj_weight.shape[1]
    assert native.supported(tr, torch.zeros(2, 5, tr.resblocks[0].attn.in_proj_weight.shape[1]), None) is False


def test_reducer_with_l0_module_raises():
    from cream_amd.tinyclip.distill import DistillStep
    from cream_amd.tinyclip.model import CLIP
    student, teacher = mirror(), G.build(CLIP)
    opt = torch.optim.SGD([p for n, p in student.named_parameters() if "l0_module" not in n], lr=0.1)
    with pytest.raises(NotImplementedError, match="l0_module"):
        DistillStep(student, teacher, opt, amp_dtype=torch.float32, reducer=object())


def mask_learning_run(device, amp_dtype):
    """Five DistillSteps per Lagrangian mode on the toy model with both l0 modules, start sparsity above the expected one (the
    term is active from step 0), then fuse_masks on 0/1-rounded masks.  Shared with the device test."""
    from cream_amd.tinyclip import distill
    from cream_amd.tinyclip.model import CLIP
    torch.manual_seed(3)
    cfg = dict(vision_cfg=dict(G.CASE["vision_cfg"]), text_cfg=dict(G.CASE["text_cfg"]))
    student = CLIP(32, **cfg, mask_image=True, mask_text=True, sparsity_warmup=4, sparsity=0.98, start_sparsity=0.9)
    teacher = CLIP(32, **cfg)
    G.fill_logas(student._image_encoder.l0_module, 5)
    G.fill_logas(student._text_encoder.l0_module, 9)
    student, teacher = student.to(device), teacher.to(device)
    opt = torch.optim.AdamW(distill.student_parameters(student), lr=1e-3)
    l0_opt = distill.make_l0_optimizer(student)
    assert not ({id(p) for g in opt.param_groups for p in g["params"]} & {id(p) for g in l0_opt.param_groups for p in g["params"]})
    assert sum(len(g["params"]) for g in l0_opt.param_groups) == 10 and [g["lr"] for g in l0_opt.param_groups] == [0.02] * 4
    assert [g["maximize"] for g in l0_opt.param_groups] == [False, True] * 2
    images, texts = (t.to(device) for t in G.inputs()[:2])
    l0i = student._image_encoder.l0_module
    for joint in (False, True):
        step = distill.DistillStep(student, teacher, opt, l0_optimizer=l0_opt, total_loss_flag=joint, amp_dtype=amp_dtype)
        lam0 = float(l0i.lambda_1.detach())
        losses, expected = [], []
        for _ in range(5):
            losses.append(float(step.step(images, texts)))
            sp = step.last_sparsity if joint else step.last_sparsity["image"]
            assert sp["target"] > sp["expected"]                    # the term is active
            expected.append(sp["expected"])
        print(f"[tinyclip l0 steps {device} joint={joint}] loss {losses[0]:.4f} -> {losses[-1]:.4f}, expected sparsity "
              f"{expected[0]:.5f} -> {expected[-1]:.5f}")
        assert all(math.isfinite(v) for v in losses), losses
        assert expected[-1] > expected[0], expected                 # towards the target
        assert float(l0i.lambda_1.detach()) > lam0                  # ascent on the multipliers
        for enc in (student._image_encoder, student._text_encoder):
            for p in enc.l0_module.z_logas.values():
                assert float(p.detach().min()) >= math.log(1e-2) - 1e-6 and float(p.detach().max()) <= math.log(1e2) + 1e-6
    _binary_masks(student)
    n0 = sum(p.numel() for p in student.parameters())
    with torch.no_grad(), step._autocast(images.device):
        student.eval()
        f0 = student(images, texts, normalized=True)
    distill.fuse_masks(student, images[:1], texts[:1])
    assert student._image_encoder.l0_module is None and student._text_encoder.l0_module is None
    assert sum(p.numel() for p in student.parameters()) < n0
    with torch.no_grad(), step._autocast(images.device):
        f1 = student(images, texts, normalized=True)
    return max(max_rel(f1[0].float().cpu(), f0[0].float().cpu()), max_rel(f1[1].float().cpu(), f0[1].float().cpu()))


def test_distill_step_learns_masks_on_cpu():
    assert mask_learning_run("cpu", torch.float32) < 1e-5           # fp32: summation order only
