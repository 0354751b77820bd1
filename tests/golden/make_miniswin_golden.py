"""Golden vectors of Mini-Swin, made by the reference's own `SwinTransformerMiniViT`
(MiniViT/Mini-Swin/models/swin_transformer_minivit.py, loaded read-only as a stand-alone module with the timm stand-ins of
tests/refshim.py):
    python tests/golden/make_miniswin_golden.py        ->  tests/golden/miniswin.{npz,json}
A two-stage model on 56 x 56 images (a shifted 2 x 2-window stage of 2 heads and a single-window stage of 4 heads, both
blocks shared twice) with the three MiniViT flags on, and the same model with the flags off (the plain shared Swin).  Seeded
weights (`miniswin_fill`, shared with the tests) and inputs; the files hold state-dict keys and shapes, the logits, and per
parameter the gradient's norm, sum and a strided sample — no weights."""
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
from fixture_utils import fill_params  # noqa: E402

STRIDE = 97
MODEL = dict(img_size=56, patch_size=4, embed_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=7, drop_path_rate=0.0,
             separate_layer_num_list=[1, 1])
MINISWIN_CASES = {
    'minivit': dict(is_sep_layernorm=True, is_transform_FFN=True, is_transform_heads=True),
    'plain': dict(is_sep_layernorm=False, is_transform_FFN=False, is_transform_heads=False),
}


def zlib_seed(s):
    return zlib.crc32(s.encode()) & 0x7fffffff


def miniswin_fill(model, seed):
    """fill_params, then: bias tables 0.3 randn, head transforms eye + 0.3 randn (non-symmetric) with 0.2 randn biases,
    every LayerNorm weight 1 + 0.1 randn."""
    fill_params(model, seed=seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            g = torch.Generator().manual_seed(zlib_seed(n) ^ seed)
            if 'relative_position_bias_table' in n:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif '.proj_l.' in n or '.proj_w.' in n:
                if p.dim() == 2:
                    p.copy_(torch.eye(p.shape[0]) + 0.3 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(0.2 * torch.randn(p.shape, generator=g))
            elif 'norm' in n and n.endswith('weight'):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))


def inputs(tag):
    g = torch.Generator().manual_seed(zlib_seed('miniswin|' + tag))
    return torch.randn(2, 3, 56, 56, generator=g), torch.randn(2, 1000, generator=g)


def digest(grads):
    out = {}
    for k in sorted(grads):
        g = grads[k].detach().double().flatten()
        out[k + '|norm'] = g.norm().reshape(1)
        out[k + '|sum'] = g.sum().reshape(1)
        out[k + '|sample'] = g[::STRIDE].clone()
    return out


def load_reference():
    import contextlib
    import importlib.util
    import io
    import refshim
    assert refshim.have_reference(), "needs the reference checkout"
    refshim._install_timm_stub()
    path = os.path.join(refshim.REFERENCE, "MiniViT", "Mini-Swin", "models", "swin_transformer_minivit.py")
    spec = importlib.util.spec_from_file_location("_ref_swin_minivit", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def make(**kw):
        with contextlib.redirect_stdout(io.StringIO()):          # the constructor prints its drop-path list
            return mod.SwinTransformerMiniViT(**kw)
    return make


def main():
    import warnings
    warnings.simplefilter("ignore")
    make = load_reference()
    outs, meta = {}, {}
    for tag, flags in MINISWIN_CASES.items():
        torch.manual_seed(0)
        model = make(**MODEL, **flags)
        miniswin_fill(model, seed=29)
        model.eval()
        x, gy = inputs(tag)
        logits = model(x)
        (logits * gy).sum().backward()
        grads = {k: p.grad for k, p in model.named_parameters()}
        assert all(v is not None for v in grads.values())
        sd = model.state_dict()
        meta[tag] = dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()],
                         n_params=sum(p.numel() for p in model.parameters()))
        outs[f'{tag}|logits'] = logits.detach().numpy()
        for k, v in digest(grads).items():
            outs[f'{tag}|{k}'] = v.numpy()
    json.dump(meta, open(os.path.join(HERE, 'miniswin.json'), 'w'), indent=1)
    np.savez_compressed(os.path.join(HERE, 'miniswin.npz'), **outs)
    print("wrote miniswin.npz", os.path.getsize(os.path.join(HERE, 'miniswin.npz')), "bytes")


if __name__ == "__main__":
    main()
