"""Fixture of TinyCLIP's mask learning (tests/golden/tinyclip_l0.npz / .json), made on the CPU by running the reference's
own classes (TinyCLIP/src/open_clip/model.py + l0module.py through tests/refshim.load_tinyclip_model): a toy CLIP whose two
towers carry an `l0_module`, on seeded weights, log-alphas and inputs.

Recorded: the hard-concrete masks sampled in training mode under `SEED`; both towers' features; a scalar loss with the two
Lagrangian terms and the gradient of every parameter (`l0_module` included; large tensors as norm / sum / strided sample);
`get_num_parameters_and_constraint(True / False)`; `lagrangian_regularization` at three steps; the eval-mode masks for
soft=True / False, `l0_mask()`, `calculate_model_size`; the pruned model's state-dict keys and shapes and its features.

    python tests/golden/make_tinyclip_l0_golden.py

The configuration, the fills and the inputs below are shared with tests/test_tinyclip_l0_cpu.py.  Weights are not stored.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from fixture_utils import grad_digest  # noqa: E402
from make_golden import tinyclip_fill, tinyclip_inputs, zlib_seed  # noqa: E402

CASE = dict(embed_dim=32, vision_cfg=dict(image_size=32, layers=2, width=128, patch_size=16),      # L = 2 * 2 + 1 = 5
            text_cfg=dict(context_length=8, vocab_size=64, width=128, heads=2, layers=2), quick_gelu=False)
MASK = dict(sparsity_warmup=10, sparsity=0.98, start_sparsity=0.9)      # above the expected sparsity: the Lagrangian term is active
SEED = 1234                 # torch seed of the training-mode forward (the hard-concrete draws)
STRIDE = 97
STEPS = (0, 5, 40)          # lagrangian_regularization: start, mid warm-up, past it
TAG = "tinyclip_l0"


def fill_logas(l0, seed):
    """Log-alphas spread around 0 so that masks of every type have zeros: N(0, 3) per entry, the four heads set by hand
    (one clearly dropped and one clearly kept per layer).  lambda_1 / lambda_2 away from their common initial value."""
    with torch.no_grad():
        for name in ("hidden_loga", "intermediate_loga"):
            p = getattr(l0, name)
            g = torch.Generator().manual_seed(zlib_seed(name) ^ seed)
            p.copy_(3.0 * torch.randn(p.shape, generator=g))
        l0.heads_loga.copy_(torch.tensor([[-4.0, 3.0], [2.5, -5.0]]))
        l0.lambda_1.fill_(7.0 + seed % 3)
        l0.lambda_2.fill_(12.0 - seed % 5)


def build(CLIP):
    """`CLIP`: the reference's class or the mirror's — same constructor arguments."""
    torch.manual_seed(0)
    model = CLIP(CASE["embed_dim"], dict(CASE["vision_cfg"]), dict(CASE["text_cfg"]), quick_gelu=CASE["quick_gelu"],
                 mask_image=True, mask_text=True, sparsity_warmup=MASK["sparsity_warmup"], sparsity=MASK["sparsity"],
                 start_sparsity=MASK["start_sparsity"])
    ie, te = model._image_encoder, model._text_encoder
    l0i, l0t = ie.l0_module, te.l0_module
    ie.l0_module = te.l0_module = None      # (the towers' fill knows nothing of the l0 parameters)
    tinyclip_fill(model, seed=41)
    ie.l0_module, te.l0_module = l0i, l0t
    fill_logas(l0i, 5)
    fill_logas(l0t, 9)
    return model


def inputs():
    return tinyclip_inputs(TAG, CASE)


def train_step(model, step=5):
    """-> (features, scale, loss, masks) after backward of the fixture's loss."""
    images, texts, gi, gt = inputs()
    model.train()
    torch.manual_seed(SEED)
    fi, ft, scale = model(images, texts, normalized=True)
    li = model._image_encoder.l0_module.lagrangian_regularization(step)[0]
    lt = model._text_encoder.l0_module.lagrangian_regularization(step)[0]
    loss = (fi * gi).sum() + (ft * gt).sum() + scale + li + lt
    loss.backward()
    return fi, ft, scale, loss, (model._image_encoder.mask, model._text_encoder.mask)


def l0_records(l0):
    """The host-side quantities of one L0Module, as {name: array or json-able}."""
    arrays, meta = {}, {}
    for hidden in (True, False):
        arrays[f"num_params|{hidden}"] = l0.get_num_parameters_and_constraint(hidden).detach().reshape(1)
    for s in STEPS:
        loss, expect, target = l0.lagrangian_regularization(s)
        assert float(loss.detach()) > 0, (s, expect, target)
        arrays[f"lagrangian|{s}"] = torch.tensor([float(loss.detach()), expect, target], dtype=torch.float64)
    l0.eval()
    for soft in (True, False):
        for k, v in l0.forward(soft=soft).items():
            arrays[f"eval|{soft}|{k}"] = v
    for k, v in l0.l0_mask().items():
        arrays[f"l0_mask|{k}"] = v
    meta["model_size"] = l0.calculate_model_size(l0.forward())
    meta["shapes"] = {k: list(v) for k, v in l0.shapes.items()}
    meta["prunable_model_size"] = l0.prunable_model_size
    l0.train()
    return arrays, meta


def fuse(model):
    """train.py:333-362 on the toy inputs: eval forward, prune(), l0_module = None."""
    images, texts, _, _ = inputs()
    with torch.no_grad():
        model.eval()
        model(images, texts)
        model._image_encoder = model._image_encoder.prune()
        model._text_encoder = model._text_encoder.prune()
    model._image_encoder.l0_module = model._text_encoder.l0_module = None
    return model


def main():
    import refshim
    m = refshim.load_tinyclip_model()
    model = build(m.CLIP)
    arrays, meta = {}, dict(keys=list(model.state_dict().keys()))
    fi, ft, scale, loss, masks = train_step(model)
    for tower, mk in zip(("image", "text"), masks):
        for k, v in mk.items():
            assert bool((v == 0).any()) and bool((v > 0).any()), (tower, k)       # exact zeros in all three mask types
            arrays[f"{tower}|train|{k}"] = v.detach()
    arrays.update({"image_features": fi.detach(), "text_features": ft.detach(), "scale": scale.detach().reshape(1),
                   "loss": loss.detach().reshape(1)})
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    arrays.update({"grad|" + k: v for k, v in grad_digest(grads, stride=STRIDE).items()})
    for tower, enc in (("image", model._image_encoder), ("text", model._text_encoder)):
        a, mt = l0_records(enc.l0_module)
        arrays.update({f"{tower}|{k}": v for k, v in a.items()})
        meta[tower] = mt
        ev = {k: v for k, v in a.items() if k.startswith("eval|True|")}
        assert all(bool((v == 0).any()) for v in ev.values()), tower                # a hidden column, a head, some units dropped
        assert bool((ev["eval|True|heads_z"].reshape(2, 2) == 0).any(dim=1).all())
    images, texts, _, _ = inputs()
    with torch.no_grad():
        model.eval()
        fi, ft, _ = model(images, texts, normalized=True)
        arrays.update({"eval|image_features": fi, "eval|text_features": ft})
    fuse(model)
    meta["pruned"] = {k: list(v.shape) for k, v in model.state_dict().items()}
    with torch.no_grad():
        fi, ft, _ = model(images, texts, normalized=True)
    arrays.update({"pruned|image_features": fi, "pruned|text_features": ft})
    json.dump(meta, open(os.path.join(HERE, "tinyclip_l0.json"), "w"), indent=1)
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(os.path.join(HERE, "tinyclip_l0.npz"), **out)
    print(f"wrote tinyclip_l0.npz: {sum(a.nbytes for a in out.values()) / 1e3:.1f} kB, {len(out)} arrays")


if __name__ == "__main__":
    main()
