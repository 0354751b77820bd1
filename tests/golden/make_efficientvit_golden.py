"""Golden vectors of EfficientViT, made by the reference's own classes (EfficientViT/classification/model/efficientvit.py and
build.py, loaded read-only as a package with the timm stand-ins of tests/refshim.py plus the two names it imports beyond them,
`timm.models.vision_transformer.trunc_normal_` and `timm.models.layers.SqueezeExcite`, added here):
    python tests/golden/make_efficientvit_golden.py        ->  tests/golden/efficientvit.{npz,json}
A three-stage model on 224 x 224 images, B = 2: four windows of 7 x 7 on the 14 x 14 map (2 heads, 32 wide), one window of
7 x 7 (3 heads, 32 wide) and one of 4 x 4 (4 heads, 16 wide), depthwise kernels 7, 5, 3, 3.  Seeded weights and BatchNorm
statistics (`efficientvit_fill`, shared with the tests) and inputs; the files hold state-dict keys and shapes, the logits in
eval mode, the logits after `replace_batchnorm`, the logits of one training-mode forward, the BatchNorm running statistics after
it and, per parameter, the norm, sum and a strided sample of that forward's gradient — no weights.  A second, forward-only
record runs the same weights at 160 x 160, whose 10 x 10 map is padded to 14.  efficientvit.json holds the small model's keys
and shapes in full, before and after `replace_batchnorm`, and for each of the six published factories, before and after, the
number of entries, the number of elements and `keys_digest` — a sha256 over every "key shape" line in state-dict order, which
pins names, order and shapes of the 214 to 835 entries of a model without 250 KB of lists.

`SqueezeExcite` is timm 0.5.4's `SEModule` (the release the reference's requirements.txt pins), written from memory of that
release: timm is not installed where this was made."""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
from fixture_utils import fill_params  # noqa: E402
from make_miniswin_golden import digest, zlib_seed  # noqa: E402  (STRIDE lives there too)

MODEL = dict(img_size=224, embed_dim=[64, 96, 64], num_heads=[2, 3, 4], depth=[1, 1, 1], kernels=[7, 5, 3, 3], num_classes=10)
PADDED = dict(MODEL, img_size=160)
FACTORIES = ("EfficientViT_M0", "EfficientViT_M1", "EfficientViT_M2", "EfficientViT_M3", "EfficientViT_M4", "EfficientViT_M5")
SEED = 41


# the BatchNorm weights the constructors set to zero, but for the attention's `proj`: the last one of every depthwise and FFN branch
ZERO_INIT = ('pw2.bn.weight', 'dw0.m.bn.weight', 'dw1.m.bn.weight')


def efficientvit_fill(model, seed=SEED):
    """fill_params, then: attention biases 0.3 randn, every BatchNorm weight 1 + 0.1 randn — the zero-initialised ones of the depthwise
    and FFN branches 0.3 times that (the attention's `proj` keeps 1: its branch is as large as the stream it is added to), so that
    every branch matters and the twenty residual sums still leave activations of order 1: with all of them at 1
    the last stage's q and k have a standard deviation near 10, the softmax saturates, and a bf16 run of the composed model is
    20 to 50 % off the fp32 logits, which measures nothing — running means 0.1 randn, running variances in [0.5, 1.5]."""
    fill_params(model, seed=seed)
    with torch.no_grad():
        for n, p in list(model.named_parameters()) + list(model.named_buffers()):
            g = torch.Generator().manual_seed(zlib_seed(n) ^ seed)
            if n.endswith('attention_biases'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif n.endswith(ZERO_INIT):
                p.copy_(0.3 * (1.0 + 0.1 * torch.randn(p.shape, generator=g)))
            elif n.endswith('bn.weight'):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith('running_mean'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith('running_var'):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
    model.train(model.training)                     # eval mode caches the gathered bias: refresh it


def inputs(tag='small', size=224):
    g = torch.Generator().manual_seed(zlib_seed('efficientvit|' + tag))
    return torch.randn(2, 3, size, size, generator=g), torch.randn(2, MODEL['num_classes'], generator=g)


class _SEModule(nn.Module):
    def __init__(self, channels, rd_ratio=1. / 16, rd_channels=None, rd_divisor=8):
        super().__init__()
        if not rd_channels:
            v = channels * rd_ratio
            rd_channels = max(rd_divisor, int(v + rd_divisor / 2) // rd_divisor * rd_divisor)       # round_limit = 0: never bumped
        self.fc1 = nn.Conv2d(channels, rd_channels, kernel_size=1, bias=True)
        self.fc2 = nn.Conv2d(rd_channels, channels, kernel_size=1, bias=True)

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * self.fc2(self.fc1(s).relu()).sigmoid()


def load_reference():
    """-> (efficientvit module, build module) of the reference."""
    import importlib.util
    import refshim
    assert refshim.have_reference(), "needs the reference checkout"
    refshim._install_timm_stub()
    sys.modules["timm.models.vision_transformer"].trunc_normal_ = sys.modules["timm.models.layers"].trunc_normal_
    sys.modules["timm.models.layers"].SqueezeExcite = _SEModule
    root = os.path.join(refshim.REFERENCE, "EfficientViT", "classification", "model")
    pkg = types.ModuleType("_ref_efficientvit")
    pkg.__path__ = [root]
    sys.modules["_ref_efficientvit"] = pkg
    mods = []
    for name in ("efficientvit", "build"):
        spec = importlib.util.spec_from_file_location(f"_ref_efficientvit.{name}", os.path.join(root, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods.append(mod)
    return tuple(mods)


def bn_stats(model):
    return {k: v for k, v in model.state_dict().items() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}


def shapes(model):
    sd = model.state_dict()
    return dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()])


def keys_digest(model):
    """-> dict(n, numel, sha256) of a model's state dict: entries, elements, and the digest of its "key shape" lines in order."""
    import hashlib
    sd = model.state_dict()
    text = "".join(f"{k} {list(v.shape)}\n" for k, v in sd.items())
    return dict(n=len(sd), numel=sum(v.numel() for v in sd.values()), sha256=hashlib.sha256(text.encode()).hexdigest())


def main():
    import warnings
    warnings.simplefilter("ignore")
    ref, build = load_reference()
    torch.manual_seed(0)
    model = ref.EfficientViT(**MODEL)
    efficientvit_fill(model)
    x, gy = inputs()
    model.eval()
    with torch.no_grad():
        outs = {'small|logits_eval': model(x).numpy()}
    model.train()
    logits = model(x)
    (logits * gy).sum().backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(v is not None for v in grads.values())
    outs['small|logits_train'] = logits.detach().numpy()
    for k, v in bn_stats(model).items():
        outs[f'small|stat|{k}'] = v.numpy()
    for k, v in digest(grads).items():
        outs[f'small|{k}'] = v.numpy()
    meta = {'small': dict(shapes(model), n_params=sum(p.numel() for p in model.parameters()))}

    torch.manual_seed(0)
    fused = ref.EfficientViT(**MODEL)
    efficientvit_fill(fused)
    fused.eval()
    build.replace_batchnorm(fused)
    with torch.no_grad():
        outs['small|logits_fused_bn'] = fused(x).numpy()
    meta['small|fused_bn'] = shapes(fused)

    torch.manual_seed(0)
    padded = ref.EfficientViT(**PADDED)
    efficientvit_fill(padded)
    padded.eval()
    with torch.no_grad():
        outs['padded|logits_eval'] = padded(inputs('padded', 160)[0]).numpy()

    for name in FACTORIES:
        m = getattr(build, name)()
        meta[name] = keys_digest(m)
        build.replace_batchnorm(m)
        meta[name + '|fused_bn'] = keys_digest(m)
    json.dump(meta, open(os.path.join(HERE, 'efficientvit.json'), 'w'), indent=None, separators=(',', ':'))
    np.savez_compressed(os.path.join(HERE, 'efficientvit.npz'), **outs)
    print("wrote efficientvit.npz", os.path.getsize(os.path.join(HERE, 'efficientvit.npz')), "bytes; efficientvit.json",
          os.path.getsize(os.path.join(HERE, 'efficientvit.json')), "bytes")


if __name__ == "__main__":
    main()
