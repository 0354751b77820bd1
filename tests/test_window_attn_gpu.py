"""Fused window attention (cream_amd/window_attn.py, csrc/window_attn.hip) and the Mini-Swin mirror on the GPU:
A. the kernels against the module's own composed branch (fp32 reference, bf16 composed as the yardstick of bf16 noise),
B. the mirror on the reference-made fixture, on the fused path,
C. the repeat index selects the LayerNorms, head transforms and the shift on the fused path,
D. bit-identical reruns,
E. what the kernels do not cover falls back to the composed branch."""
import os
from contextlib import contextmanager

import pytest
import torch

from helpers import max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = {"window_attn_fwd", "window_attn_bwd"}


@contextmanager
def fused_off():
    old = os.environ.get("CREAM_IRPE_FUSED")
    os.environ["CREAM_IRPE_FUSED"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CREAM_IRPE_FUSED"]
        else:
            os.environ["CREAM_IRPE_FUSED"] = old


class Layer(torch.nn.Module):
    """One repeat of a block's attention half — norm1, qkv, window attention, proj — through the block's own code."""

    def __init__(self, H, res, window, shift, mix, attn_drop=0.0, seed=0):
        super().__init__()
        from cream_amd import miniswin
        torch.manual_seed(seed)
        self.shift = shift
        self.blk = miniswin.SwinTransformerBlock(H * 32, res, H, window_size=window, shift_size=window // 2, drop_path=[0.],
                                                 attn_drop=attn_drop, is_transform_heads=mix)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for n, p in self.blk.named_parameters():
                if 'relative_position_bias_table' in n:
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
                elif n.startswith('proj_l') or n.startswith('proj_w'):
                    # eye + 0.3 randn: non-symmetric, so [o,h] / [h,o] or swapped transforms show; nonzero biases
                    p.copy_(torch.eye(H) + 0.3 * torch.randn(H, H, generator=g) if p.dim() == 2 else 0.2 * torch.randn(H, generator=g))
                elif n == 'attn.qkv.bias':
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
        self.blk.mlp = torch.nn.Identity()                    # the attention half alone: x + attn(x), then x + x
        self.blk.norm2 = torch.nn.Identity()

    def forward(self, x):
        return self.blk.forward_feature(x, is_shift=self.shift > 0, layer_index=0)


def tensors_of(m):
    b = m.blk
    out = {"d qkv.weight": b.attn.qkv.weight.grad, "d table": b.attn.relative_position_bias_table.grad}
    if b.proj_l is not None:
        out.update({"d proj_l.weight": b.proj_l[0].weight.grad, "d proj_w.weight": b.proj_w[0].weight.grad,
                    "d proj_w.bias": b.proj_w[0].bias.grad, "d proj_l.bias": b.proj_l[0].bias.grad})
    return out


def run_layer(m, x, gy, autocast, fused):
    """-> ({name: tensor}, regions seen)"""
    from cream_amd import timing
    m.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    timing.reset()
    timing.enable(True)
    try:
        if fused:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = m(x)
        else:
            with fused_off(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = m(x)
        (y.float() * gy).sum().backward()
    finally:
        timing.enable(False)
    res = {"out": y.detach().float().cpu(), "dx": x.grad.detach().float().cpu()}
    res.update({k: v.detach().float().cpu() for k, v in tensors_of(m).items()})
    return res, set(timing.summary())


def max_heads_mixed():
    from cream_amd import window_attn
    return window_attn.MAX_HEADS_MIXED


CASES = {
    # all four mask patterns incl. the nine-region corner window, wrap-around addressing, table scatter across windows and images
    "shifted_mixed": dict(H=3, res=(14, 14), shift=3, mix=True, B=2),
    "rect_plain": dict(H=4, res=(14, 21), shift=0, mix=False, B=2),           # non-square map, independent heads
    "rect_shifted": dict(H=2, res=(21, 14), shift=3, mix=True, B=1),          # shift on a non-square map (swapped axes show)
    "single_window": dict(H=6, res=(7, 7), shift=0, mix=True, B=3),           # window = map, shift disabled
    "mixed_max": dict(H=None, res=(14, 14), shift=3, mix=True, B=1),          # largest exchange buffer
    "plain_32": dict(H=32, res=(7, 7), shift=0, mix=False, B=2),              # largest head count
    "one_head": dict(H=1, res=(14, 14), shift=3, mix=True, B=1),              # 1 x 1 mixes
    # 640 work items: more than the persistent grids have workgroups, so a workgroup loops over items and its partial sums them
    "many_items": dict(H=2, res=(14, 14), shift=3, mix=True, B=80),
    # other window sizes through the module: one key tile (w = 4), 64 keys without padding (w = 8); 12 heads = three head slots
    "window4": dict(H=3, res=(8, 12), shift=2, mix=True, B=2, window=4),
    "window8": dict(H=3, res=(16, 24), shift=4, mix=True, B=2, window=8),
    "mixed_12": dict(H=12, res=(14, 14), shift=3, mix=True, B=2),
}


def case_of(tag):
    c = dict(CASES[tag])
    if c["H"] is None:
        c["H"] = max_heads_mixed()
    return c


def case_inputs(c, seed=5):
    g = torch.Generator().manual_seed(seed)
    E, L = c["H"] * 32, c["res"][0] * c["res"][1]
    x = torch.randn(c["B"], L, E, generator=g).bfloat16().float().to(DEV)          # the same bf16-rounded input for all
    gy = torch.randn(c["B"], L, E, generator=g).to(DEV)
    return x, gy


def make_layer(c, window=None, **kw):
    window = window or c.get("window", 7)
    m = Layer(c["H"], c["res"], window, c["shift"], c["mix"], **kw).to(DEV)
    if c["shift"] == 0 and m.blk.shift_size > 0:
        # an unshifted, unmasked layer (plain Swin's even blocks): the reference's shared block would still pass its mask
        m.blk.shift_size = 0
        m.blk.attn_mask = None
    return m


@pytest.mark.parametrize("tag", list(CASES))
def test_fused_against_composed(tag):
    """err(fused) <= max(2 err(composed bf16), 2^-7) for every tensor, both against the fp32 composed branch; d proj_l.bias
    (zero in exact arithmetic: the softmax is shift-invariant) absolutely, max|fused| <= max(2 max|composed bf16|,
    2^-7 max|d proj_l.weight (fp32)|)."""
    c = case_of(tag)
    m = make_layer(c)
    assert (m.blk.attn_mask is not None) == (c["shift"] > 0)
    x, gy = case_inputs(c)
    ref, names_a = run_layer(m, x, gy, autocast=False, fused=True)        # fp32: the module itself stays composed
    comp, names_b = run_layer(m, x, gy, autocast=True, fused=False)
    fus, names_c = run_layer(m, x, gy, autocast=True, fused=True)
    assert not NEW & names_a and not NEW & names_b, (names_a, names_b)
    assert NEW <= names_c, names_c
    bad = []
    for k in ref:
        if k == "d proj_l.bias":
            eb, ec = float(comp[k].abs().max()), float(fus[k].abs().max())
            bound = max(2 * eb, 2.0 ** -7 * float(ref["d proj_l.weight"].abs().max()))
        else:
            eb, ec = max_rel(comp[k], ref[k]), max_rel(fus[k], ref[k])
            bound = max(2 * eb, 2.0 ** -7)
        print(f"[window_attn {tag}] {k:16s} composed bf16 {eb:.3e}  fused {ec:.3e}  bound {bound:.3e}")
        if not ec <= bound:
            bad.append((k, eb, ec))
    assert not bad, bad


@pytest.mark.parametrize("tag", ["minivit", "plain"])
def test_whole_model_on_fixture_takes_the_fused_path(tag):
    """Every block of the fixture model is covered (2 and 4 heads of 32, window 7): no composed attention may run — then
    no (B nW, H, N, N) softmax does.  Error against the reference-made fixture within twice the composed bf16 run's."""
    from test_miniswin import build, errors, fixture, run
    from cream_amd import timing
    model = build(tag).to(DEV)
    with fused_off():
        logits_c, grads_c = run(model, tag, DEV, autocast=True)
    grads_c = {k: v.detach().clone() for k, v in grads_c.items()}
    calls = []
    hooks = [m.attn.softmax.register_forward_hook(lambda *a: calls.append(1)) for layer in model.layers for m in layer.blocks]
    timing.reset()
    timing.enable(True)
    logits_f, grads_f = run(model, tag, DEV, autocast=True)
    timing.enable(False)
    for h in hooks:
        h.remove()
    s = timing.summary()
    assert NEW <= set(s) and not calls, (set(s), len(calls))
    assert s["window_attn_fwd"]["launches"] == 4 and s["window_attn_bwd"]["launches"] == 4      # 2 stages x 2 repeats
    (ec, zc), (ef, zf) = errors(tag, logits_c, grads_c), errors(tag, logits_f, grads_f)
    bad = {k: (ec[k], ef[k]) for k in ef if not ef[k] <= max(2 * ec[k], 2.0 ** -7)}
    fix = fixture()
    for k in zf:                                          # d proj_l.bias: absolutely, on the scale of d proj_l.weight
        scale = float(fix[f"{tag}|{k[:-4]}weight|norm"][0])
        if not zf[k] <= max(2 * zc[k], 2.0 ** -7 * scale):
            bad[k] = (zc[k], zf[k])
    print(f"[miniswin gpu bf16 {tag}] worst composed {max(ec.values()):.2e} fused {max(ef.values()):.2e}")
    assert not bad, bad


def test_repeat_index_selects_the_instances_on_the_fused_path():
    """Repeat 0 and repeat 1 differ (norms, transforms, shift): each repeat on the fused path equals the same repeat on the
    composed path within bf16 noise, is far from the other repeat, and reacts to its own instances only."""
    from cream_amd import miniswin, timing
    torch.manual_seed(1)
    blk = miniswin.SwinTransformerBlock(64, (14, 14), 2, window_size=7, shift_size=3, drop_path=[0., 0.], is_sep_layernorm=True,
                                        is_transform_heads=True).eval()
    with torch.no_grad():
        blk.attn.relative_position_bias_table.normal_(std=0.3)
        for r in range(2):
            blk.norm1_list[r].weight.copy_(1.0 + 0.3 * torch.randn(64))
            for lst in (blk.proj_l, blk.proj_w):
                lst[r].weight.copy_(torch.eye(2) + 0.3 * torch.randn(2, 2))
                lst[r].bias.copy_(0.2 * torch.randn(2))
    blk.mlp = torch.nn.Identity()                        # out = 2 (x + attention): the attention half alone
    blk.norm2_list = torch.nn.ModuleList([torch.nn.Identity(), torch.nn.Identity()])
    blk = blk.to(DEV)
    x = torch.randn(2, 196, 64, device=DEV)

    def att(y):
        return (y.float() / 2 - x).cpu()
    timing.reset()
    timing.enable(True)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        fused = [blk.forward_feature(x, is_shift=bool(r), layer_index=r) for r in range(2)]
        with fused_off():
            comp = [blk.forward_feature(x, is_shift=bool(r), layer_index=r) for r in range(2)]
            whole_c = blk(x)
        whole = blk(x)
        for r in range(2):
            assert max_rel(att(fused[r]), att(comp[r])) < 3e-2, r
        assert max_rel(att(fused[0]), att(comp[1])) > 0.2
        assert max_rel(whole.float().cpu(), whole_c.float().cpu()) < 3e-2
        # the shift of the call, not the block's: repeat 1 without its roll differs
        assert max_rel(att(blk.forward_feature(x, is_shift=False, layer_index=1)), att(comp[1])) > 0.05
        # repeat 1's transforms are read by repeat 1 only
        blk.proj_w[1].weight.zero_()
        assert torch.equal(blk.forward_feature(x, is_shift=False, layer_index=0), fused[0])
        assert not torch.equal(blk.forward_feature(x, is_shift=True, layer_index=1), fused[1])
        blk.proj_l[0].bias.add_(1.0)                      # a constant before the softmax: no effect, but read
        blk.norm1_list[0].weight.zero_()
        assert not torch.equal(blk.forward_feature(x, is_shift=False, layer_index=0), fused[0])
    timing.enable(False)
    assert "window_attn_fwd" in set(timing.summary())


def test_reruns_are_bit_identical():
    c = case_of("shifted_mixed")
    m = make_layer(c)
    x, gy = case_inputs(c)
    a, names = run_layer(m, x, gy, autocast=True, fused=True)
    b, _ = run_layer(m, x, gy, autocast=True, fused=True)
    assert NEW <= names
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("what", ["window12", "fp32", "dropout_training", "switch", "too_many_mixed_heads"])
def test_uncovered_configurations_stay_composed(what):
    """Composed, and still right: equal to the composed branch selected by the switch, and within bf16 noise of fp32."""
    H = max_heads_mixed() + 1 if what == "too_many_mixed_heads" else 2
    window, res = (12, (12, 24)) if what == "window12" else (7, (7, 14))
    c = dict(H=H, res=res, shift=window // 2, mix=True, B=1)
    m = make_layer(c, window=window, attn_drop=0.1 if what == "dropout_training" else 0.0)
    m.train(what == "dropout_training")
    x, gy = case_inputs(c)
    autocast = what != "fp32"
    torch.manual_seed(11)
    if what == "switch":
        with fused_off():
            a, names = run_layer(m, x, gy, autocast=autocast, fused=True)
    else:
        a, names = run_layer(m, x, gy, autocast=autocast, fused=True)
    assert not NEW & names, names
    torch.manual_seed(11)
    b, _ = run_layer(m, x, gy, autocast=autocast, fused=False)            # the composed branch, selected by the switch
    for k in a:
        assert torch.equal(a[k], b[k]), k
    if what != "dropout_training":
        m.eval()
        ref, _ = run_layer(m, x, gy, autocast=False, fused=False)
        for k in ("out", "dx", "d qkv.weight", "d table"):
            assert max_rel(a[k], ref[k]) < (1e-5 if what == "fp32" else 4e-2), (k, max_rel(a[k], ref[k]))


def test_eval_mode_with_attn_drop_takes_the_fused_path():
    c = dict(H=2, res=(7, 14), shift=3, mix=True, B=1)
    m = make_layer(c, attn_drop=0.1).eval()
    x, gy = case_inputs(c)
    _, names = run_layer(m, x, gy, autocast=True, fused=True)
    assert NEW <= names, names
