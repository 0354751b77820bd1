"""Golden vectors of S3 (AutoFormerV2), made by the reference's own `SSSTransformer` (AutoFormerV2/model/SSS.py, loaded
read-only as a stand-alone module with the timm stand-ins of tests/refshim.py):
    python tests/golden/make_s3_golden.py        ->  tests/golden/s3.{npz,json}
A two-stage model on 56 x 56 images with patch 2: a 28 x 28 map of 2 x 2 windows of 14 x 14 (two blocks of 2 heads, the
second shifted by 7 and masked), merged to a 14 x 14 map that is one 14 x 14 window (two blocks of 4 heads, no shift left after
the clamp); the blocks of a stage differ in their MLP ratio.  Seeded weights (`miniswin_fill`, shared with the tests) and
inputs; the files hold state-dict keys and shapes, the logits, and per parameter the gradient's norm, sum and a strided sample
— no weights.  s3.json also holds the keys and shapes of the three published configurations, built by the reference from the
values of its configs/S3-{T,S,B}.yaml (read here as data; the values themselves are recorded under 'configs')."""
import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
from make_miniswin_golden import digest, miniswin_fill, zlib_seed  # noqa: E402,F401  (STRIDE lives there too)

MODEL = dict(img_size=56, patch_size=2, num_classes=1000, embed_dim=[64, 128], depths=[2, 2], num_heads=[[2, 2], [4, 4]],
             window_size=[[14, 14], [14, 14]], mlp_ratio=[[4.0, 2.0], [3.0, 4.0]], drop_path_rate=0.0)
SEED = 31


def inputs():
    g = torch.Generator().manual_seed(zlib_seed('s3|small'))
    return torch.randn(2, 3, 56, 56, generator=g), torch.randn(2, 1000, generator=g)


def load_reference():
    import importlib.util
    import refshim
    assert refshim.have_reference(), "needs the reference checkout"
    refshim._install_timm_stub()
    path = os.path.join(refshim.REFERENCE, "AutoFormerV2", "model", "SSS.py")
    spec = importlib.util.spec_from_file_location("_ref_sss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SSSTransformer


def published(size):
    """The five lists of configs/S3-{size}.yaml: one `KEY: [literal]` per line."""
    import refshim
    cfg = {}
    with open(os.path.join(refshim.REFERENCE, "AutoFormerV2", "configs", f"S3-{size}.yaml")) as fh:
        for line in fh:
            if ':' in line:
                key, val = line.split(':', 1)
                cfg[key.strip()] = ast.literal_eval(val.strip())
    return dict(embed_dim=cfg['EMBED_DIM'], depths=cfg['DEPTHS'], num_heads=cfg['NUM_HEADS'], window_size=cfg['WINDOW_SIZE'],
                mlp_ratio=cfg['MLP_RATIO'])


def main():
    import warnings
    warnings.simplefilter("ignore")
    make = load_reference()
    torch.manual_seed(0)
    model = make(**MODEL)
    miniswin_fill(model, seed=SEED)
    model.eval()
    x, gy = inputs()
    logits = model(x)
    (logits * gy).sum().backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(v is not None for v in grads.values())
    sd = model.state_dict()
    meta = {'small': dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()],
                          n_params=sum(p.numel() for p in model.parameters())), 'configs': {}}
    outs = {'small|logits': logits.detach().numpy()}
    for k, v in digest(grads).items():
        outs[f'small|{k}'] = v.numpy()
    for size in 'TSB':
        cfg = published(size)
        sd = make(img_size=224, patch_size=4, num_classes=1000, **cfg).state_dict()
        meta['configs'][size] = cfg
        meta[size] = dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()])
    json.dump(meta, open(os.path.join(HERE, 's3.json'), 'w'), indent=None, separators=(',', ':'))
    np.savez_compressed(os.path.join(HERE, 's3.npz'), **outs)
    print("wrote s3.npz", os.path.getsize(os.path.join(HERE, 's3.npz')), "bytes; s3.json",
          os.path.getsize(os.path.join(HERE, 's3.json')), "bytes")


if __name__ == "__main__":
    main()
