"""Mini-Swin (cream_amd/miniswin.py, cream_amd/window_attn.py) without a device, against fixtures made by running the
reference's own `SwinTransformerMiniViT` (tests/golden/make_miniswin_golden.py): state-dict keys and shapes, parameter count,
logits and the gradient of every parameter on the composed fp32 path; the shift alternation of a shared block; the
`usable_window` truth table; the C ABI's argument checks."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from helpers import load_json, load_npz, max_rel  # noqa: E402
from make_miniswin_golden import MINISWIN_CASES, MODEL, STRIDE, inputs, miniswin_fill  # noqa: E402


def build(tag):
    from cream_amd import miniswin
    torch.manual_seed(0)
    model = miniswin.SwinTransformerMiniViT(**MODEL, **MINISWIN_CASES[tag])
    miniswin_fill(model, seed=29)
    return model.eval()


def run(model, tag, device, autocast=False):
    x, gy = inputs(tag)
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = model(x.to(device))
    (logits.float() * gy.to(device)).sum().backward()
    return logits, {k: p.grad for k, p in model.named_parameters()}


_FIX = {}


def fixture():
    if not _FIX:
        _FIX.update(load_npz("miniswin.npz"))
    return _FIX


def errors(tag, logits, grads):
    """-> ({name: error}, {name: |g|}) against the fixture: logits by max_rel, gradients by norm and by the strided sample
    scaled with the tensor's own magnitude.  A gradient that is zero in exact arithmetic (proj_l.bias: the softmax is
    shift-invariant; the reference's value is rounding noise) comes back in the second dict, as its own norm."""
    fix = fixture()
    errs = {"logits": max_rel(logits.detach().cpu().float(), fix[f"{tag}|logits"])}
    zeros = {}
    for k, v in fix.items():
        if k.startswith(tag + "|") and k.endswith("|norm"):
            name = k[len(tag) + 1:-5]
            ref = float(v[0])
            g = grads[name].detach().cpu().double().flatten()
            if ref < 1e-5:
                zeros[name] = float(g.norm())
                continue
            errs[name + "|norm"] = abs(float(g.norm()) - ref) / ref
            scale = ref / max(1.0, g.numel()) ** 0.5
            sample = torch.from_numpy(fix[f"{tag}|{name}|sample"])
            errs[name + "|sample"] = float((g[::STRIDE] - sample).abs().max() / scale) / 10.0
    return errs, zeros


def compare(tag, logits, grads, tol):
    errs, zeros = errors(tag, logits, grads)
    bad = {k: e for k, e in {**errs, **zeros}.items() if not e <= tol}
    assert not bad, f"{tag}: exceeds {tol}: " + ", ".join(f"{k}={e:.2e}" for k, e in sorted(bad.items(), key=lambda t: -t[1])[:8])
    return max(errs.values())


@pytest.mark.parametrize("tag", list(MINISWIN_CASES))
def test_state_dict_matches_the_reference(tag):
    model = build(tag)
    meta = load_json("miniswin.json")[tag]
    sd = model.state_dict()
    assert list(sd.keys()) == meta["keys"]
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    assert sum(p.numel() for p in model.parameters()) == meta["n_params"]
    if tag == "minivit":
        for k in ("layers.0.blocks.0.attn_mask", "layers.0.blocks.0.attn.relative_position_index",
                  "layers.0.blocks.0.norm1_list.1.weight", "layers.0.blocks.0.proj_l.1.bias", "layers.0.blocks.0.proj_w.0.weight",
                  "layers.1.blocks.0.local_norm_list.0.bias", "layers.1.blocks.0.local_conv_list.1.weight"):
            assert k in sd, k
        assert "layers.1.blocks.0.attn_mask" not in sd          # one window: no shift, no mask
    else:
        assert model.layers[0].blocks[0].proj_l is None and model.layers[0].blocks[0].proj_w is None


@pytest.mark.parametrize("tag", list(MINISWIN_CASES))
def test_composed_fp32_matches_the_reference_on_cpu(tag):
    model = build(tag)
    logits, grads = run(model, tag, "cpu")
    worst = compare(tag, logits, grads, 1e-4)
    print(f"[miniswin cpu {tag}] worst {worst:.2e}")


def test_buffers_match_the_reference_constructions():
    """relative_position_index and attn_mask from their closed forms: rel(i,j) = (iy-jy+w-1)(2w-1) + (ix-jx+w-1); the mask
    separates the three slices per axis [0, H-w), [H-w, H-s), [H-s, H) of the shifted frame."""
    from cream_amd import miniswin
    w, H, W, s = 7, 14, 21, 3
    idx = miniswin.relative_position_index(w, w)
    for i, j in ((0, 0), (0, 48), (48, 0), (10, 30), (33, 5)):
        iy, ix, jy, jx = i // w, i % w, j // w, j % w
        assert int(idx[i, j]) == (iy - jy + w - 1) * (2 * w - 1) + (ix - jx + w - 1)
    assert int(idx.min()) == 0 and int(idx.max()) == (2 * w - 1) ** 2 - 1
    mask = miniswin.shift_mask(H, W, w, s)
    assert mask.shape == (6, 49, 49) and set(mask.unique().tolist()) == {0.0, -100.0}

    def region(p, n):
        return 0 if p < n - w else (1 if p < n - s else 2)
    for win in range(6):
        wy, wx = win // 3, win % 3
        for i, j in ((0, 48), (3, 4), (20, 28), (24, 25), (48, 6)):
            ri = (region(wy * w + i // w, H), region(wx * w + i % w, W))
            rj = (region(wy * w + j // w, H), region(wx * w + j % w, W))
            assert float(mask[win, i, j]) == (0.0 if ri == rj else -100.0)
    assert float(mask[0].abs().max()) == 0.0 and len({float(v) for v in mask[5].unique()}) == 2


def test_shift_alternates_per_repeat(monkeypatch):
    """A block shared three times rolls the map in every other repeat, starting from is_init_window_shift, and undoes the
    roll; the mask goes to the attention in every repeat."""
    from cream_amd import miniswin
    for init in (False, True):
        torch.manual_seed(0)
        blk = miniswin.SwinTransformerBlock(32, (14, 14), 1, window_size=7, shift_size=3, drop_path=[0., 0., 0.],
                                            is_init_window_shift=init, is_sep_layernorm=True, is_transform_heads=True).eval()
        rolls, masks = [], []
        real_roll, real_attend = torch.roll, blk.attn.attend
        monkeypatch.setattr(torch, "roll", lambda x, shifts, dims: (rolls.append(tuple(shifts)), real_roll(x, shifts, dims))[1])
        monkeypatch.setattr(blk.attn, "attend", lambda q, mask=None, **k: (masks.append(mask is not None), real_attend(q, mask=mask, **k))[1])
        seen = []
        real_ff = blk.forward_feature
        monkeypatch.setattr(blk, "forward_feature", lambda x, s=False, i=0: (seen.append((bool(s), i)), real_ff(x, s, i))[1])
        with torch.no_grad():
            blk(torch.randn(1, 196, 32))
        monkeypatch.undo()
        assert seen == [(init, 0), (not init, 1), (init, 2)]
        assert rolls == [(-3, -3), (3, 3)] * (2 if init else 1)
        assert masks == [True, True, True]
    layer = miniswin.BasicLayer(32, (14, 14), depth=6, num_heads=1, window_size=7, drop_path=[0.] * 6, separate_layer_num=2)
    assert [b.is_init_window_shift for b in layer.blocks] == [False, True] and [b.share_num for b in layer.blocks] == [3, 3]


def test_factory_recipes():
    from cream_amd import miniswin
    m = miniswin.mini_swin('tiny', num_classes=10)
    assert [len(layer.blocks) for layer in m.layers] == [1, 1, 1, 1]
    assert [layer.blocks[0].share_num for layer in m.layers] == [2, 2, 6, 2]
    assert [layer.blocks[0].num_heads for layer in m.layers] == [3, 6, 12, 24]
    assert m.layers[3].blocks[0].shift_size == 0 and m.layers[3].blocks[0].attn_mask is None
    assert m.layers[0].blocks[0].proj_l is not None and m.layers[0].blocks[0].local_conv_list is not None
    s, b = miniswin.mini_swin('small', num_classes=10), miniswin.mini_swin('base', num_classes=10)
    assert [len(layer.blocks) for layer in s.layers] == [1, 1, 9, 1] and [len(layer.blocks) for layer in b.layers] == [1, 1, 9, 1]
    assert [layer.blocks[0].num_heads for layer in b.layers] == [4, 8, 16, 32] and b.embed_dim == 128


def test_usable_window_truth_table(monkeypatch):
    from cream_amd import window_attn as W
    monkeypatch.delenv("CREAM_IRPE_FUSED", raising=False)
    bf, dev = torch.bfloat16, "cuda:0"

    def table(H, w=7, dtype=torch.float32):
        return torch.zeros((2 * w - 1) ** 2, H, dtype=dtype)

    def lin(H, dtype=torch.float32, bias=True):
        return torch.nn.Linear(H, H, bias=bias).to(dtype)

    assert W.MAX_HEADS == 32 and W.MAX_HEADS_MIXED == 16
    assert W.usable_window(bf, dev, 32, 3, 7, table(3))
    assert W.usable_window(bf, dev, 32, 3, 7, table(3), lin(3), lin(3))
    assert W.usable_window(bf, dev, 32, 32, 7, table(32))                              # plain Swin-B's last stage
    assert W.usable_window(bf, dev, 32, 16, 7, table(16), lin(16), lin(16))            # Mini-Swin-B stage 3
    assert W.usable_window(bf, dev, 32, 1, 8, table(1, 8))                             # 64 tokens
    # the 7x7 last stage of Mini-Swin-S / -B with head transforms stays composed (LDS and register budget)
    assert not W.usable_window(bf, dev, 32, 24, 7, table(24), lin(24), lin(24))
    assert not W.usable_window(bf, dev, 32, 32, 7, table(32), lin(32), lin(32))
    assert not W.usable_window(bf, dev, 32, 17, 7, table(17), lin(17), lin(17))
    assert not W.usable_window(bf, dev, 32, 33, 7, table(33))
    assert not W.usable_window(bf, dev, 32, 0, 7, table(0))
    assert not W.usable_window(torch.float32, dev, 32, 3, 7, table(3))
    assert not W.usable_window(torch.float16, dev, 32, 3, 7, table(3))
    assert not W.usable_window(bf, "cpu", 32, 3, 7, table(3))
    assert not W.usable_window(bf, dev, 64, 3, 7, table(3))
    assert not W.usable_window(bf, dev, 32, 3, 12, table(3, 12))                       # window 12: 144 tokens
    assert not W.usable_window(bf, dev, 32, 3, 9, table(3, 9))
    assert not W.usable_window(bf, dev, 32, 3, 7, table(3), dropout_p=0.1)
    assert not W.usable_window(bf, dev, 32, 3, 7, table(3, dtype=torch.bfloat16))
    assert not W.usable_window(bf, dev, 32, 3, 7, table(3).t().contiguous().t())        # not contiguous
    assert not W.usable_window(bf, dev, 32, 3, 7, table(4))
    assert not W.usable_window(bf, dev, 32, 3, 7, table(3), lin(3, torch.bfloat16), lin(3))
    assert not W.usable_window(bf, dev, 32, 3, 7, table(3), lin(3), lin(3, bias=False))
    assert not W.usable_window(bf, dev, 32, 3, 7, table(3), lin(3), None)
    bad = lin(3)
    bad.weight = torch.nn.Parameter(torch.zeros(3, 6)[:, ::2])
    assert not W.usable_window(bf, dev, 32, 3, 7, table(3), bad, lin(3))
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")
    assert not W.usable_window(bf, dev, 32, 3, 7, table(3))


def _desc(**kw):
    from cream_amd import _lib
    d = _lib.WindowAttnDesc()
    d.q, d.k, d.v, d.out, d.lse, d.table = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    d.sb, d.sn, d.sh = 196 * 288, 288, 32
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = 2, 3, 14, 14, 7, 3, 3, 32
    d.scale = 32 ** -0.5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_c_abi_argument_checks_return_codes_without_a_launch():
    from cream_amd import _lib
    lib = _lib.load()
    ok = lambda d, bwd=0: lib.cream_window_attn_check(ctypes.byref(d), bwd)          # noqa: E731
    assert ok(_desc()) == 0
    assert lib.cream_window_attn_check(None, 0) == -1
    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(lse=None), dict(table=None),
                dict(head_dim=64), dict(w=9, Hs=18, Ws=18), dict(w=0), dict(Hs=15), dict(Ws=20), dict(Hs=0), dict(shift=7),
                dict(shift=-1), dict(mask_shift=7), dict(H=0), dict(H=33), dict(B=-1), dict(sn=284), dict(q=0x1008),
                dict(wl=0x7000), dict(wl=0x7000, bl=0x7100, ww=0x7200)):
        d = _desc(**bad)
        assert ok(d) == -1, bad
        assert lib.cream_window_attn_fwd(ctypes.byref(d), None) == -1, bad            # the same check, before any HIP call
        assert lib.cream_window_attn_bwd(ctypes.byref(d), None) == -1, bad
    mixed = dict(wl=0x7000, bl=0x7100, ww=0x7200, bw=0x7300)
    assert ok(_desc(**mixed)) == 0 and ok(_desc(H=16, sn=3 * 16 * 32, sb=196 * 3 * 16 * 32, **mixed)) == 0
    assert ok(_desc(H=17, sn=3 * 17 * 32, **mixed)) == -1                             # beyond MAX_HEADS_MIXED
    assert ok(_desc(H=32, sn=3 * 32 * 32, sb=196 * 3 * 32 * 32)) == 0
    assert ok(_desc(Hs=14, Ws=21, sb=294 * 288)) == 0 and ok(_desc(w=8, Hs=8, Ws=16, shift=0, mask_shift=0)) == 0
    # backward: its own pointers
    full = dict(dout=0x8000, dq=0x9000, dk=0xa000, dv=0xb000, dsb=196 * 288, dsn=288, dsh=32, delta=0xc000, part=0xd000, part_blocks=4)
    assert ok(_desc(**full), 1) == 0
    for k in ("dout", "dq", "dk", "dv", "delta", "part"):
        assert ok(_desc(**{**full, k: None}), 1) == -1, k
    assert ok(_desc(**{**full, "part_blocks": 0}), 1) == -1
    # an empty batch is a no-op success, forward and backward, and launches nothing
    assert lib.cream_window_attn_fwd(ctypes.byref(_desc(B=0)), None) == 0
    assert lib.cream_window_attn_bwd(ctypes.byref(_desc(B=0, **full)), None) == 0
    # partial size: [(2w-1)^2 H | H H | H H | H | H]
    assert lib.cream_window_attn_part_size(3, 7, 0) == 169 * 3
    assert lib.cream_window_attn_part_size(3, 7, 1) == 169 * 3 + 2 * 9 + 6
    assert lib.cream_window_attn_part_size(3, 9, 0) == -1 and lib.cream_window_attn_part_size(0, 7, 0) == -1
