"""S3 (cream_amd/s3.py, cream_amd/window_attn_large.py) without a device, against fixtures made by running the reference's own
`SSSTransformer` (tests/golden/make_s3_golden.py): state-dict keys and shapes of the small model and of the three published
configurations, logits and the gradient of every parameter on the composed fp32 path; the clamped window of a small map; the
`usable_large_window` truth table; the C ABI's argument checks; `evaluate`."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from helpers import load_json, load_npz, max_rel  # noqa: E402
from make_miniswin_golden import STRIDE, miniswin_fill  # noqa: E402
from make_s3_golden import MODEL, SEED, inputs  # noqa: E402

TAG = "small"


def build():
    from cream_amd import s3
    torch.manual_seed(0)
    model = s3.SSSTransformer(**MODEL)
    miniswin_fill(model, seed=SEED)
    return model.eval()


def run(model, device, autocast=False):
    x, gy = inputs()
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = model(x.to(device))
    (logits.float() * gy.to(device)).sum().backward()
    return logits, {k: p.grad for k, p in model.named_parameters()}


_FIX = {}


def fixture():
    if not _FIX:
        _FIX.update(load_npz("s3.npz"))
    return _FIX


def errors(logits, grads):
    """-> {name: error} against the fixture, as tests/test_miniswin.py measures them: logits by max_rel, gradients by norm and
    by the strided sample scaled with the tensor's own magnitude."""
    fix = fixture()
    errs = {"logits": max_rel(logits.detach().cpu().float(), fix[f"{TAG}|logits"])}
    for k, v in fix.items():
        if k.startswith(TAG + "|") and k.endswith("|norm"):
            name = k[len(TAG) + 1:-5]
            ref = float(v[0])
            assert ref > 1e-5, name                               # no gradient of this model is zero in exact arithmetic
            g = grads[name].detach().cpu().double().flatten()
            errs[name + "|norm"] = abs(float(g.norm()) - ref) / ref
            scale = ref / max(1.0, g.numel()) ** 0.5
            sample = torch.from_numpy(fix[f"{TAG}|{name}|sample"])
            errs[name + "|sample"] = float((g[::STRIDE] - sample).abs().max() / scale) / 10.0
    return errs


def test_state_dict_matches_the_reference():
    model = build()
    meta = load_json("s3.json")[TAG]
    sd = model.state_dict()
    assert list(sd.keys()) == meta["keys"]
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    assert sum(p.numel() for p in model.parameters()) == meta["n_params"]
    assert "layers.0.blocks.1.attn_mask" in sd and "layers.0.blocks.0.attn_mask" not in sd
    assert "layers.1.blocks.1.attn_mask" not in sd              # one window: no shift, no mask
    assert tuple(sd["layers.0.blocks.0.attn.qkv.weight"].shape) == (2 * 32 * 3, 64)
    assert tuple(sd["layers.0.downsample.reduction.weight"].shape) == (128, 256)        # out_dim, not 2 dim
    assert tuple(sd["layers.0.blocks.1.mlp.fc1.weight"].shape) == (128, 64)             # the block's own MLP ratio


@pytest.mark.parametrize("size", ["T", "S", "B"])
def test_published_configurations_match_the_reference(size):
    from cream_amd import s3
    meta = load_json("s3.json")
    pub = meta["configs"][size]                                   # S3-T lists 8 values for the 6 blocks of stage 3: the model reads 6
    used = {k: [row[:d] for row, d in zip(v, pub["depths"])] if isinstance(v[0], list) else v for k, v in pub.items()}
    assert s3.s3_config(size) == used                            # the factory restates the published lists
    with torch.device("meta"):
        # on the meta device nothing is allocated or initialised (S3-B has 71 M parameters)
        model = s3.s3(size)
    sd = model.state_dict()
    assert list(sd.keys()) == meta[size]["keys"]
    assert [list(v.shape) for v in sd.values()] == meta[size]["shapes"]
    if size == "S":                                               # 7 x 7 map under window 14: clamped before the table is built
        blk = model.layers[3].blocks[1]
        assert blk.window_size == 7 and blk.shift_size == 0 and blk.attn_mask is None
        assert tuple(blk.attn.relative_position_bias_table.shape) == (13 * 13, 24)
        assert tuple(model.layers[0].blocks[1].attn_mask.shape) == (16, 196, 196)
    assert [b.window_size for b in model.layers[2].blocks] == [14] * len(model.layers[2].blocks)
    assert [b.shift_size for b in model.layers[2].blocks[:2]] == [0, 0]                  # 14 x 14 map: one window


def test_composed_fp32_matches_the_reference_on_cpu():
    model = build()
    logits, grads = run(model, "cpu")
    errs = errors(logits, grads)
    bad = {k: e for k, e in errs.items() if not e <= 1e-4}
    print(f"[s3 cpu] worst {max(errs.values()):.2e}")
    assert not bad, sorted(bad.items(), key=lambda t: -t[1])[:8]


def test_usable_large_window_truth_table(monkeypatch):
    from cream_amd import window_attn_large as W
    monkeypatch.delenv("CREAM_IRPE_FUSED", raising=False)
    bf, dev = torch.bfloat16, "cuda:0"

    def table(H, w=14, dtype=torch.float32):
        return torch.zeros((2 * w - 1) ** 2, H, dtype=dtype)

    assert (W.MIN_WINDOW, W.MAX_WINDOW, W.MAX_HEADS, W.HEAD_DIM) == (9, 14, 32, 32)
    assert not W.usable_large_window(bf, dev, 32, 3, 8, table(3, 8))
    assert not W.usable_large_window(bf, dev, 32, 3, 15, table(3, 15))
    assert W.usable_large_window(bf, dev, 32, 3, 9, table(3, 9))
    assert W.usable_large_window(bf, dev, 32, 3, 14, table(3))
    assert W.usable_large_window(bf, dev, 32, 12, 14, table(12))                        # S3 stage 3
    assert W.usable_large_window(bf, dev, 32, 32, 12, table(32, 12))                    # Swin-B-384's last stage
    assert W.usable_large_window(bf, dev, 32, 1, 14, table(1))
    assert not W.usable_large_window(torch.float32, dev, 32, 3, 14, table(3))
    assert not W.usable_large_window(torch.float16, dev, 32, 3, 14, table(3))
    assert not W.usable_large_window(bf, "cpu", 32, 3, 14, table(3))
    assert not W.usable_large_window(bf, dev, 64, 3, 14, table(3))
    assert not W.usable_large_window(bf, dev, 32, 0, 14, table(0))
    assert not W.usable_large_window(bf, dev, 32, 33, 14, table(33))
    assert not W.usable_large_window(bf, dev, 32, 3, 14, table(3).t().contiguous().t())   # not contiguous
    assert not W.usable_large_window(bf, dev, 32, 3, 14, table(4))
    assert not W.usable_large_window(bf, dev, 32, 3, 14, table(3, 13))
    assert not W.usable_large_window(bf, dev, 32, 3, 14, table(3, dtype=torch.bfloat16))
    assert not W.usable_large_window(bf, dev, 32, 3, 14, None)
    assert not W.usable_large_window(bf, dev, 32, 3, 14, table(3), dropout_p=0.1)
    assert W.usable_large_window(bf, dev, 32, 3, 14, table(3), dropout_p=0.0)
    assert [W.padded_tokens(w) for w in range(9, 15)] == [96, 128, 128, 160, 192, 224]
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")
    assert not W.usable_large_window(bf, dev, 32, 3, 14, table(3))


def _desc(**kw):
    from cream_amd import _lib
    d = _lib.WindowAttnLargeDesc()
    d.q, d.k, d.v, d.out, d.lse, d.table = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    d.sb, d.sn, d.sh = 784 * 288, 288, 32
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = 2, 3, 28, 28, 14, 7, 7, 32
    d.scale = 32 ** -0.5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_c_abi_argument_checks_return_codes_without_a_launch():
    from cream_amd import _lib
    lib = _lib.load()
    ok = lambda d, bwd=0: lib.cream_window_attn_large_check(ctypes.byref(d), bwd)    # noqa: E731
    assert ok(_desc()) == 0
    assert lib.cream_window_attn_large_check(None, 0) == -1
    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(lse=None), dict(table=None),
                dict(head_dim=64), dict(w=8, Hs=16, Ws=16), dict(w=7), dict(w=15, Hs=30, Ws=30), dict(w=0), dict(Hs=29), dict(Ws=30),
                dict(Hs=0), dict(shift=14), dict(shift=-1), dict(mask_shift=14), dict(mask_shift=-1), dict(H=0), dict(H=33),
                dict(B=-1), dict(sn=284), dict(q=0x1008)):
        d = _desc(**bad)
        assert ok(d) == -1, bad
        assert lib.cream_window_attn_large_fwd(ctypes.byref(d), None) == -1, bad      # the same check, before any HIP call
        assert lib.cream_window_attn_large_bwd(ctypes.byref(d), None) == -1, bad
    assert ok(_desc(H=32, sn=3 * 32 * 32, sb=784 * 3 * 32 * 32)) == 0 and ok(_desc(H=1)) == 0
    for w in range(9, 15):
        assert ok(_desc(w=w, Hs=2 * w, Ws=3 * w, shift=w - 1, mask_shift=0)) == 0, w
    assert ok(_desc(Hs=14, Ws=14, shift=0, mask_shift=0)) == 0
    # backward: its own pointers
    full = dict(dout=0x8000, dq=0x9000, dk=0xa000, dv=0xb000, dsb=784 * 288, dsn=288, dsh=32, delta=0xc000, part=0xd000, part_blocks=4)
    assert ok(_desc(**full), 1) == 0
    for k in ("dout", "dq", "dk", "dv", "delta", "part"):
        assert ok(_desc(**{**full, k: None}), 1) == -1, k
    assert ok(_desc(**{**full, "part_blocks": 0}), 1) == -1
    # an empty batch is a no-op success, forward and backward, and launches nothing
    assert lib.cream_window_attn_large_fwd(ctypes.byref(_desc(B=0)), None) == 0
    assert lib.cream_window_attn_large_bwd(ctypes.byref(_desc(B=0, **full)), None) == 0
    assert lib.cream_window_attn_large_blocks(ctypes.byref(_desc(B=0))) == 0
    assert lib.cream_window_attn_large_blocks(ctypes.byref(_desc(w=8, Hs=16, Ws=16))) == -1
    # partial size: (2w-1)^2 H
    assert lib.cream_window_attn_large_part_size(3, 14) == 729 * 3 and lib.cream_window_attn_large_part_size(32, 9) == 289 * 32
    for H, w in ((3, 8), (3, 15), (0, 14), (33, 14)):
        assert lib.cream_window_attn_large_part_size(H, w) == -1, (H, w)


def test_evaluate_counts_what_the_reference_counts():
    """Loss averaged over the batches, accuracies over the samples (AutoFormerV2/engine.py:36-46), on a model whose logits are
    known: batches of 3 and 1 samples."""
    from cream_amd import s3

    class Fixed(torch.nn.Module):
        def forward(self, x):
            return x.flatten(1)[:, :8]

    def batch(rows, target):
        x = torch.zeros(len(rows), 1, 1, 8)
        for i, top in enumerate(rows):
            for rank, cls in enumerate(top):
                x[i, 0, 0, cls] = 8.0 - rank
        return x, torch.tensor(target)

    loader = [batch([[0, 1, 2, 3, 4, 5], [1, 0, 2, 3, 4, 5], [7, 6, 5, 4, 3, 2]], [0, 0, 0]), batch([[2, 3, 4, 5, 6, 7]], [2])]
    res = s3.evaluate(Fixed(), loader, "cpu")
    assert res["acc1"] == pytest.approx(50.0) and res["acc5"] == pytest.approx(75.0)
    losses = [float(torch.nn.functional.cross_entropy(x.flatten(1), t)) for x, t in loader]
    assert res["loss"] == pytest.approx(sum(losses) / 2, rel=1e-6)
