"""TinyViT (cream_amd/tinyvit.py, cream_amd/token_conv.py) without a device, against fixtures made by running the reference's
own `TinyViT` (tests/golden/make_tinyvit_golden.py): state-dict keys and shapes of the small model and of the five published
factories; logits (eval and training mode), the gradient of every parameter and the BatchNorm running statistics on the
composed fp32 path; the padded map; `expand_offset_bias`; the truth table of the path decisions; the C ABI's argument checks."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from helpers import load_json, load_npz, max_rel  # noqa: E402
from make_miniswin_golden import STRIDE  # noqa: E402
from make_tinyvit_golden import FACTORIES, MODEL, PADDED, inputs, tinyvit_fill  # noqa: E402

TAG = "small"
# zero in exact arithmetic: a per-channel constant on the stage's output, which PatchMerging's 1 x 1 convolution carries into a
# training-mode BatchNorm, whose mean subtraction removes it
ZERO = {"layers.1.blocks.1.mlp.fc2.bias"}


def build(cfg=MODEL, **kw):
    from cream_amd import tinyvit
    torch.manual_seed(0)
    model = tinyvit.TinyViT(**cfg, **kw)
    tinyvit_fill(model)
    return model


_FIX = {}


def fixture():
    if not _FIX:
        _FIX.update(load_npz("tinyvit.npz"))
    return _FIX


def run_eval(model, device, autocast=False):
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        return model(inputs()[0].to(device))


def run_train(model, device, autocast=False):
    """One training-mode forward and backward -> (logits, {name: gradient}); the running statistics move."""
    x, gy = inputs()
    model.train()
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = model(x.to(device))
    (logits.float() * gy.to(device)).sum().backward()
    return logits, {k: p.grad for k, p in model.named_parameters()}


def errors(logits, grads):
    """-> {name: error} of a training-mode step against the fixture, as tests/test_s3.py measures them."""
    fix = fixture()
    errs = {"logits": max_rel(logits.detach().cpu().float(), fix[f"{TAG}|logits_train"])}
    for k, v in fix.items():
        if k.startswith(TAG + "|") and k.endswith("|norm"):
            name = k[len(TAG) + 1:-5]
            ref = float(v[0])
            g = grads[name].detach().cpu().double().flatten()
            if name in ZERO:                                      # measured against the sibling weight's gradient
                assert ref < 1e-5, name
                errs[name + "|zero"] = float(g.norm()) / float(fix[f"{TAG}|{name[:-4]}weight|norm"][0])
                continue
            assert ref > 1e-5, name
            errs[name + "|norm"] = abs(float(g.norm()) - ref) / ref
            scale = ref / max(1.0, g.numel()) ** 0.5
            errs[name + "|sample"] = float((g[::STRIDE] - torch.from_numpy(fix[f"{TAG}|{name}|sample"])).abs().max() / scale) / 10.0
    return errs


def stat_errors(model):
    """-> {buffer: max_rel} of the BatchNorm buffers against the fixture's after one training forward."""
    fix, sd = fixture(), model.state_dict()
    out = {}
    for k, v in fix.items():
        if k.startswith(TAG + "|stat|"):
            name = k[len(TAG) + 6:]
            out[name] = max_rel(sd[name].detach().cpu().double(), v)
    assert len(out) >= 3 * 9
    return out


def test_state_dict_matches_the_reference():
    model = build()
    meta = load_json("tinyvit.json")[TAG]
    sd = model.state_dict()
    assert list(sd.keys()) == meta["keys"]
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    assert sum(p.numel() for p in model.parameters()) == meta["n_params"]
    assert not any("attention_bias_idxs" in k or "_fold" in k or "_expand" in k for k in sd)
    assert tuple(sd["layers.1.blocks.0.attn.attention_biases"].shape) == (2, 49)
    assert tuple(sd["layers.2.blocks.1.attn.attention_biases"].shape) == (3, 196)
    assert tuple(sd["layers.1.blocks.0.local_conv.c.weight"].shape) == (64, 1, 3, 3)
    assert model.no_weight_decay_keywords() == {"attention_biases"}


@pytest.mark.parametrize("name", FACTORIES)
def test_published_factories_match_the_reference(name):
    from cream_amd import tinyvit
    meta = load_json("tinyvit.json")[name]
    with torch.device("meta"):
        model = getattr(tinyvit, name)()
    sd = model.state_dict()
    assert list(sd.keys()) == meta["keys"]
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    for p in model.parameters():
        assert hasattr(p, "lr_scale") and hasattr(p, "param_name")


def test_attention_bias_idxs_are_the_reference_enumeration():
    """The vectorised index against the reference's loop (offsets numbered in the order they are met), non-square included."""
    import itertools
    from cream_amd import tinyvit
    for res in ((1, 1), (2, 3), (7, 7), (3, 2)):
        pts = list(itertools.product(range(res[0]), range(res[1])))
        seen, idxs = {}, []
        for p1 in pts:
            for p2 in pts:
                off = (abs(p1[0] - p2[0]), abs(p1[1] - p2[1]))
                idxs.append(seen.setdefault(off, len(seen)))
        a = tinyvit.Attention(32, 32, 1, attn_ratio=1, resolution=res)
        assert a.attention_biases.shape[1] == len(seen)
        assert torch.equal(a.attention_bias_idxs, torch.tensor(idxs).view(len(pts), len(pts)))


def test_layer_lr_decay_scales():
    model = build(layer_lr_decay=0.5)
    depth = sum(MODEL["depths"])
    p = dict(model.named_parameters())
    assert p["patch_embed.seq.0.c.weight"].lr_scale == 0.5 ** (depth - 1) == p["layers.0.blocks.0.conv1.c.weight"].lr_scale
    assert p["layers.0.downsample.conv1.c.weight"].lr_scale == 0.5 ** (depth - 1)
    assert p["layers.1.blocks.1.attn.attention_biases"].lr_scale == 0.5 ** (depth - 3)
    assert p["head.weight"].lr_scale == 1.0 and p["head.weight"].param_name == "head.weight"


def test_composed_fp32_matches_the_reference_on_cpu():
    fix = fixture()
    model = build()
    e_eval = max_rel(run_eval(model, "cpu").float(), fix[f"{TAG}|logits_eval"])
    logits, grads = run_train(model, "cpu")
    errs = dict(errors(logits, grads), logits_eval=e_eval, **{"stat|" + k: v for k, v in stat_errors(model).items()})
    print(f"[tinyvit cpu] worst {max(errs.values()):.2e}")
    bad = {k: e for k, e in errs.items() if not e <= 1e-3}
    assert not bad, sorted(bad.items(), key=lambda t: -t[1])[:8]
    assert int(model.state_dict()["layers.1.blocks.0.local_conv.bn.num_batches_tracked"]) == 1


def test_padded_map_matches_the_reference_on_cpu():
    model = build(PADDED).eval()
    assert model.layers[1].blocks[0].input_resolution == (20, 20) and model.layers[2].blocks[0].input_resolution == (10, 10)
    with torch.no_grad():
        logits = model(inputs("padded", 160)[0])
    e = max_rel(logits.float(), fixture()["padded|logits_eval"])
    print(f"[tinyvit cpu padded] {e:.2e}")
    assert e <= 1e-3


def test_use_checkpoint_computes_the_same():
    a, b = build(), build(use_checkpoint=True)
    (la, ga), (lb, gb) = run_train(a, "cpu"), run_train(b, "cpu")
    assert torch.equal(la, lb)
    worst = {k: max_rel(gb[k], ga[k]) for k in ga if k not in ZERO}        # the recomputation may sum in another order
    assert max(worst.values()) <= 1e-5, sorted(worst.items(), key=lambda t: -t[1])[:4]


def test_train_quirk_caches_the_bias_when_leaving_training_mode():
    from cream_amd import tinyvit
    a = tinyvit.Attention(64, 32, 2, attn_ratio=1, resolution=(7, 7))
    with torch.no_grad():
        a.attention_biases.normal_()
    a.eval()
    assert torch.equal(a.ab, a.attention_biases[:, a.attention_bias_idxs]) and not a.ab.requires_grad
    assert torch.equal(a.ab_table, tinyvit.expand_offset_bias(a.attention_biases, 7)) and not a.ab_table.requires_grad
    old = a.ab.clone()
    with torch.no_grad():
        a.attention_biases.add_(1.0)
    assert torch.equal(a.ab, old)                                  # as the reference: stale until training mode is left again
    a.train()
    assert not hasattr(a, "ab") and a.ab_table is None
    a.eval()
    assert torch.equal(a.ab, old + 1.0)


# ---- expand_offset_bias -------------------------------------------------------------------------------------------------------
def _swin_index(w):
    from cream_amd.miniswin import relative_position_index
    return relative_position_index(w, w)


@pytest.mark.parametrize("w", [1, 2, 7, 12, 14])
def test_expand_offset_bias(w):
    from cream_amd import tinyvit
    H, N = 3, w * w
    g = torch.Generator().manual_seed(100 + w)
    att = tinyvit.Attention(H * 32, 32, H, attn_ratio=1, resolution=(w, w))
    ab = torch.randn(H, N, generator=g).requires_grad_(True)
    gout = torch.randn(H, N, N, generator=g)
    # forward: through Swin's index it is the reference's gather, bit for bit
    table = tinyvit.expand_offset_bias(ab, w)
    assert table.shape == ((2 * w - 1) ** 2, H) and table.dtype == torch.float32 and table.is_contiguous()
    via_swin = table[_swin_index(w).view(-1)].view(N, N, H).permute(2, 0, 1)
    assert torch.equal(via_swin, ab[:, att.attention_bias_idxs])
    # every offset is read by at most 4 entries, every entry reads one offset
    src, fold, valid = tinyvit.offset_bias_index(w)
    assert int(valid.sum()) == (2 * w - 1) ** 2 and sorted(fold[valid].tolist()) == list(range((2 * w - 1) ** 2))
    assert torch.equal(src[fold[valid]], torch.arange(N).view(-1, 1).expand(N, 4)[valid])
    # backward: the fold against fp64 autograd of the reference's gather, to fp32 rounding of sums of <= 4 N terms
    (via_swin * gout).sum().backward()
    got = ab.grad.clone()
    ab64 = ab.detach().double().requires_grad_(True)
    (ab64[:, att.attention_bias_idxs] * gout.double()).sum().backward()
    absum = torch.zeros(H, N, dtype=torch.float64).index_add_(1, att.attention_bias_idxs.view(-1), gout.double().abs().view(H, -1))
    assert bool(((got.double() - ab64.grad).abs() <= 4 * N * 2.0 ** -24 * absum + 1e-30).all())
    # two runs of the fold alone are bit-identical
    gt = torch.randn((2 * w - 1) ** 2, H, generator=g)
    runs = []
    for _ in range(2):
        a = ab.detach().clone().requires_grad_(True)
        tinyvit.expand_offset_bias(a, w).backward(gt)
        runs.append(a.grad)
    assert torch.equal(runs[0], runs[1])
    ref = torch.zeros(N, H, dtype=torch.float64).index_add_(0, src, gt.double()).t()
    assert bool(((runs[0].double() - ref).abs() <= 4 * 2.0 ** -24 * torch.zeros(N, H, dtype=torch.float64).index_add_(0, src, gt.double().abs()).t()).all())


# ---- the path decisions -------------------------------------------------------------------------------------------------------
def _block(window=7, res=(28, 28), heads=2, **kw):
    from cream_amd import tinyvit
    return tinyvit.TinyViTBlock(heads * 32, res, heads, window_size=window, **kw)


def test_path_decision_truth_table(monkeypatch):
    monkeypatch.delenv("CREAM_IRPE_FUSED", raising=False)
    bf, f32, dev = torch.bfloat16, torch.float32, "cuda:0"
    kind = lambda blk, dtype=bf, device=dev: blk.attention_kind(dtype, device)[0]          # noqa: E731
    assert kind(_block()) == "small" and kind(_block(14, (14, 14), 3)) == "large" and kind(_block(12, (24, 36))) == "large"
    assert kind(_block(8, (16, 16))) == "small" and kind(_block(9, (18, 18))) == "large"
    table = _block(14, (14, 14), 3).attention_kind(bf, dev)[1]
    assert tuple(table.shape) == (27 * 27, 3) and table.requires_grad                         # training mode: from the parameter
    assert _block().eval().attention_kind(bf, dev)[1].requires_grad is False                    # eval: the cached table
    assert kind(_block(), f32) is None                                                         # fp32 stays composed
    assert kind(_block(), bf, "cpu") is None                                                   # CPU stays composed
    assert kind(_block(7, (20, 20))) is None and kind(_block(14, (10, 10), 3)) is None          # a padded map stays composed
    assert kind(_block(24, (24, 24), 12)) is None                                              # w = 24 of the 384 model
    assert kind(_block(16, (32, 32), 6)) is None and kind(_block(32, (32, 32), 12)) is None     # the 512 model
    from cream_amd import tinyvit
    assert kind(tinyvit.TinyViTBlock(128, (28, 28), 2, window_size=7)) is None                  # 64-wide heads
    # the convolution: a device, bf16 or fp32, the constructor / module switch
    blk = _block()
    assert blk.fused_local_conv and blk.conv_is_fused(bf, dev) and blk.conv_is_fused(f32, dev)
    assert not blk.conv_is_fused(f32, "cpu") and not blk.conv_is_fused(torch.float16, dev)
    assert not _block(fused_local_conv=False).conv_is_fused(bf, dev)
    blk.fused_local_conv = False
    assert not blk.conv_is_fused(bf, dev)
    assert not _block(local_conv_size=5).conv_is_fused(bf, dev)
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")                                                # the attention only
    assert kind(_block()) is None and kind(_block(14, (14, 14), 3)) is None
    assert _block().conv_is_fused(bf, dev)
    model = build()
    assert model.fused_local_conv
    model.fused_local_conv = False
    assert not any(b.fused_local_conv for layer in model.layers[1:] for b in layer.blocks)
    assert not build(fused_local_conv=False).fused_local_conv


def test_usable_token_conv_truth_table():
    from cream_amd.token_conv import usable_token_conv as ok
    bf, dev = torch.bfloat16, "cuda:0"
    assert ok(bf, dev, 64, 3, 1, 1, 1, 64) and ok(torch.float32, dev, 576, (3, 3), (1, 1), (1, 1), (1, 1), 576) and ok(bf, dev, 8, 3, 1, 1, 1, 8)
    assert not ok(bf, "cpu", 64, 3, 1, 1, 1, 64) and not ok(torch.float16, dev, 64, 3, 1, 1, 1, 64)
    assert not ok(bf, dev, 60, 3, 1, 1, 1, 60) and not ok(bf, dev, 0, 3, 1, 1, 1, 0)
    assert not ok(bf, dev, 64, 3, 1, 1, 1, 1) and not ok(bf, dev, 64, 3, 1, 1, 1, 32)            # not depthwise
    assert not ok(bf, dev, 64, 7, 1, 3, 1, 64) and not ok(bf, dev, 64, 3, 2, 1, 1, 64)
    assert not ok(bf, dev, 64, 3, 1, 0, 1, 64) and not ok(bf, dev, 64, 3, 1, 1, 2, 64) and not ok(bf, dev, 64, (3, 1), 1, 1, 1, 64)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def _desc(**kw):
    from cream_amd import _lib
    d = _lib.TokenDwconv3Desc()
    d.x, d.w, d.bias, d.y = 0x1000, 0x2000, 0x3000, 0x4000
    d.B, d.Hs, d.Ws, d.C, d.dtype = 2, 5, 9, 64, _lib.BF16
    d.dy, d.dx, d.part, d.part_blocks = 0x5000, 0x6000, 0x7000, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_c_abi_argument_checks_return_codes_without_a_launch():
    from cream_amd import _lib
    lib = _lib.load()
    fwd = lambda d: lib.cream_token_dwconv3_fwd(ctypes.byref(d), None)           # noqa: E731
    bwd = lambda d: lib.cream_token_dwconv3_bwd(ctypes.byref(d), None)           # noqa: E731
    assert lib.cream_token_dwconv3_fwd(None, None) == -1 and lib.cream_token_dwconv3_bwd(None, None) == -1
    assert lib.cream_token_dwconv3_blocks(None) == -1
    for bad in (dict(x=None), dict(w=None), dict(C=60), dict(C=0), dict(C=-8), dict(B=0), dict(B=-1), dict(Hs=0), dict(Ws=0), dict(Ws=-3),
                dict(x=0x1008), dict(w=0x2004), dict(bias=0x3002)):
        assert fwd(_desc(**bad)) == -1 and bwd(_desc(**bad)) == -1, bad
    for bad in (dict(y=None), dict(y=0x4008)):
        assert fwd(_desc(**bad)) == -1, bad
    for bad in (dict(dy=None), dict(dx=None), dict(part=None), dict(part_blocks=0), dict(dy=0x5008), dict(dx=0x6002), dict(part=0x7004)):
        assert bwd(_desc(**bad)) == -1, bad
    for dt in (_lib.F16, _lib.F64, 7):
        assert fwd(_desc(dtype=dt)) == -2 and bwd(_desc(dtype=dt)) == -2 and lib.cream_token_dwconv3_blocks(ctypes.byref(_desc(dtype=dt))) == -2
    assert fwd(_desc(B=1 << 20, Hs=1 << 10, Ws=1 << 10)) == -4
    assert lib.cream_token_dwconv3_blocks(ctypes.byref(_desc(C=12))) == -1
    assert lib.cream_token_dwconv3_part_size(64) == 640 and lib.cream_token_dwconv3_part_size(576) == 5760
    for C in (0, -8, 12, 7):
        assert lib.cream_token_dwconv3_part_size(C) == -1, C


def test_byte_counts_from_shapes():
    from cream_amd import token_conv
    assert token_conv.fwd_bytes(2, 45, 64, 2, True) == 2 * 2 * 45 * 64 * 2 + 10 * 64 * 4
    assert token_conv.bwd_bytes(2, 45, 64, 4, 3) == 4 * 2 * 45 * 64 * 4 + 9 * 64 * 4 + 3 * 10 * 64 * 4
