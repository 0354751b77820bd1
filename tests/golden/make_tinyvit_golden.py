"""Golden vectors of TinyViT, made by the reference's own `TinyViT` (TinyViT/models/tiny_vit.py, loaded read-only as a
stand-alone module with the timm stand-ins of tests/refshim.py plus the two it imports beyond them, `timm.__version__` and
`build_model_with_cfg`):
    python tests/golden/make_tinyvit_golden.py        ->  tests/golden/tinyvit.{npz,json}
A three-stage model on 224 x 224 images, B = 2: a 56 x 56 MBConv stage, 16 windows of 7 x 7 on 28 x 28 (two blocks of 2 heads)
and one 14 x 14 window (two blocks of 3 heads).  Seeded weights and BatchNorm statistics (`tinyvit_fill`, shared with the tests)
and inputs; the files hold state-dict keys and shapes, the logits in eval mode, the logits of one training-mode forward, the
BatchNorm running statistics after it and, per parameter, the norm, sum and a strided sample of that forward's gradient — no
weights.  A second, forward-only record runs the same weights at 160 x 160: its 20 x 20 map is padded to 21 and its 10 x 10 map
to 14.  tinyvit.json also holds the keys and shapes of the five published factories as the reference builds them."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
from fixture_utils import fill_params  # noqa: E402
from make_miniswin_golden import digest, zlib_seed  # noqa: E402  (STRIDE lives there too)

MODEL = dict(img_size=224, num_classes=10, embed_dims=[32, 64, 96], depths=[1, 2, 2], num_heads=[1, 2, 3], window_sizes=[7, 7, 14],
             drop_path_rate=0.0)
PADDED = dict(MODEL, img_size=160)
FACTORIES = ("tiny_vit_5m_224", "tiny_vit_11m_224", "tiny_vit_21m_224", "tiny_vit_21m_384", "tiny_vit_21m_512")
SEED = 37


def tinyvit_fill(model, seed=SEED):
    """fill_params, then: attention biases 0.3 randn, every LayerNorm and BatchNorm weight 1 + 0.1 randn, running means
    0.1 randn, running variances in [0.5, 1.5]."""
    fill_params(model, seed=seed)
    with torch.no_grad():
        for n, p in list(model.named_parameters()) + list(model.named_buffers()):
            g = torch.Generator().manual_seed(zlib_seed(n) ^ seed)
            if n.endswith('attention_biases'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif n.endswith(('norm.weight', 'norm_head.weight', 'bn.weight')):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith('running_mean'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith('running_var'):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))


def inputs(tag='small', size=224):
    g = torch.Generator().manual_seed(zlib_seed('tinyvit|' + tag))
    return torch.randn(2, 3, size, size, generator=g), torch.randn(2, MODEL['num_classes'], generator=g)


def load_reference():
    import importlib.util
    import refshim
    assert refshim.have_reference(), "needs the reference checkout"
    refshim._install_timm_stub()
    timm = sys.modules["timm"]
    timm.__version__ = "0.4.12"
    # what tiny_vit.py asks of timm's builder when nothing is downloaded: construct the class from the model's own arguments
    timm.models.helpers.build_model_with_cfg = lambda cls, variant, pretrained, default_cfg=None, pretrained_filter_fn=None, **kw: cls(**kw)
    path = os.path.join(refshim.REFERENCE, "TinyViT", "models", "tiny_vit.py")
    spec = importlib.util.spec_from_file_location("_ref_tiny_vit", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bn_stats(model):
    return {k: v for k, v in model.state_dict().items() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}


def main():
    import warnings
    warnings.simplefilter("ignore")
    ref = load_reference()
    torch.manual_seed(0)
    model = ref.TinyViT(**MODEL)
    tinyvit_fill(model)
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
    sd = model.state_dict()
    meta = {'small': dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()],
                          n_params=sum(p.numel() for p in model.parameters()))}

    torch.manual_seed(0)
    padded = ref.TinyViT(**PADDED)
    tinyvit_fill(padded)
    padded.eval()
    with torch.no_grad():
        outs['padded|logits_eval'] = padded(inputs('padded', 160)[0]).numpy()

    for name in FACTORIES:
        sd = getattr(ref, name)().state_dict()
        meta[name] = dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()])
    json.dump(meta, open(os.path.join(HERE, 'tinyvit.json'), 'w'), indent=None, separators=(',', ':'))
    np.savez_compressed(os.path.join(HERE, 'tinyvit.npz'), **outs)
    print("wrote tinyvit.npz", os.path.getsize(os.path.join(HERE, 'tinyvit.npz')), "bytes; tinyvit.json",
          os.path.getsize(os.path.join(HERE, 'tinyvit.json')), "bytes")


if __name__ == "__main__":
    main()
