"""S3 (cream_amd/s3.py) on the GPU, on the fused window attention for 9x9 .. 14x14 windows (cream_amd/window_attn_large.py):
A. one block's attention half against its own composed branch (fp32 reference, bf16 composed as the yardstick of bf16 noise),
B. the mirror on the reference-made fixture, on the fused path: no composed attention runs,
C. what the kernels do not cover stays composed, bit for bit,
D. `evaluate` counts the same on both paths."""
import os
from contextlib import contextmanager

import pytest
import torch

from helpers import max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LARGE = {"window_attn_large_fwd", "window_attn_large_bwd"}
SMALL = {"window_attn_fwd", "window_attn_bwd"}


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
    """A block's attention half — norm1, qkv, window attention, proj — through the block's own code."""

    def __init__(self, H, res, window, shift, attn_drop=0.0, seed=0):
        super().__init__()
        from cream_amd import s3
        torch.manual_seed(seed)
        self.blk = s3.SwinTransformerBlock(H * 32, res, H, window_size=window, shift_size=shift, attn_drop=attn_drop)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            self.blk.attn.relative_position_bias_table.copy_(0.3 * torch.randn(self.blk.attn.relative_position_bias_table.shape, generator=g))
            self.blk.attn.qkv.bias.copy_(0.1 * torch.randn(self.blk.attn.qkv.bias.shape, generator=g))
        self.blk.mlp = torch.nn.Identity()                    # the attention half alone: x + attn(x), then x + x
        self.blk.norm2 = torch.nn.Identity()

    def forward(self, x):
        return self.blk(x)


def run_layer(m, x, gy, autocast, fused):
    """-> ({name: tensor}, regions seen, softmax calls of the composed branch)"""
    from cream_amd import timing
    m.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    calls = []
    hook = m.blk.attn.softmax.register_forward_hook(lambda *a: calls.append(1))
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
        hook.remove()
    res = {"out": y, "dx": x.grad, "d qkv.weight": m.blk.attn.qkv.weight.grad, "d table": m.blk.attn.relative_position_bias_table.grad}
    return {k: v.detach().float().cpu() for k, v in res.items()}, set(timing.summary()), len(calls)


CASES = {
    # 2 x 2 windows of 14 x 14, rolled by 7: all four mask patterns, wrap-around addressing, the table summed over windows and images
    "w14_shifted": dict(H=2, res=(28, 28), window=14, shift=7, B=2),
    "single_window": dict(H=3, res=(14, 14), window=14, shift=7, B=3),         # window = map: the block drops the shift
    "w12_rect": dict(H=2, res=(24, 36), window=12, shift=6, B=1),              # non-square map (swapped axes show)
}


def case_inputs(c, seed=5):
    g = torch.Generator().manual_seed(seed)
    E, L = c["H"] * 32, c["res"][0] * c["res"][1]
    x = torch.randn(c["B"], L, E, generator=g).bfloat16().float().to(DEV)          # the same bf16-rounded input for all
    gy = torch.randn(c["B"], L, E, generator=g).to(DEV)
    return x, gy


def make_layer(c, **kw):
    return Layer(c["H"], c["res"], c["window"], c["shift"], **kw).to(DEV)


@pytest.mark.parametrize("tag", list(CASES))
def test_fused_against_composed(tag):
    """err(fused) <= max(2 err(composed bf16), 2^-7) for out, dx, d qkv.weight and d table, both against the fp32 composed
    branch."""
    c = CASES[tag]
    m = make_layer(c)
    assert (m.blk.attn_mask is not None) == (tag != "single_window") and m.blk.window_size == c["window"]
    x, gy = case_inputs(c)
    ref, names_a, calls_a = run_layer(m, x, gy, autocast=False, fused=True)        # fp32: the module itself stays composed
    comp, names_b, calls_b = run_layer(m, x, gy, autocast=True, fused=False)
    fus, names_c, calls_c = run_layer(m, x, gy, autocast=True, fused=True)
    assert not (LARGE | SMALL) & (names_a | names_b) and (calls_a, calls_b) == (1, 1), (names_a, names_b)
    assert LARGE <= names_c and not SMALL & names_c and calls_c == 0, (names_c, calls_c)
    bad = []
    for k in ref:
        eb, ec = max_rel(comp[k], ref[k]), max_rel(fus[k], ref[k])
        bound = max(2 * eb, 2.0 ** -7)
        print(f"[s3 layer {tag}] {k:14s} composed bf16 {eb:.3e}  fused {ec:.3e}  bound {bound:.3e}")
        if not ec <= bound:
            bad.append((k, eb, ec))
    assert not bad, bad


def test_whole_model_on_fixture_takes_the_fused_path():
    """Every block of the fixture model is covered (2 and 4 heads of 32, window 14): no composed attention may run — then no
    (B nW, H, N, N) softmax does — and only the new regions appear.  The logits stay within twice the composed bf16 run's
    error against the reference-made fixture; the gradients within max(twice that run's, 2^-7)."""
    from test_s3 import build, errors, run
    from cream_amd import timing
    model = build().to(DEV)
    with fused_off():
        logits_c, grads_c = run(model, DEV, autocast=True)
    grads_c = {k: v.detach().clone() for k, v in grads_c.items()}
    calls = []
    hooks = [m.attn.softmax.register_forward_hook(lambda *a: calls.append(1)) for layer in model.layers for m in layer.blocks]
    timing.reset()
    timing.enable(True)
    logits_f, grads_f = run(model, DEV, autocast=True)
    timing.enable(False)
    for h in hooks:
        h.remove()
    s = timing.summary()
    assert LARGE <= set(s) and not SMALL & set(s) and not calls, (set(s), len(calls))
    assert s["window_attn_large_fwd"]["launches"] == 4 and s["window_attn_large_bwd"]["launches"] == 4      # 2 stages x 2 blocks
    ec, ef = errors(logits_c, grads_c), errors(logits_f, grads_f)
    print(f"[s3 gpu bf16] logits: composed {ec['logits']:.3e} fused {ef['logits']:.3e}; worst gradient figure: composed "
          f"{max(v for k, v in ec.items() if k != 'logits'):.2e} fused {max(v for k, v in ef.items() if k != 'logits'):.2e}")
    assert ef["logits"] <= 2 * ec["logits"], (ec["logits"], ef["logits"])
    bad = {k: (ec[k], ef[k]) for k in ef if not ef[k] <= max(2 * ec[k], 2.0 ** -7)}
    assert not bad, bad


def test_small_windows_of_a_model_take_the_existing_kernels():
    """A stage with window 7 next to one with window 14 (S3-T, S3-B): the first goes through window_attn, the second through
    window_attn_large, nothing is composed."""
    from cream_amd import s3, timing
    torch.manual_seed(0)
    model = s3.SSSTransformer(img_size=56, patch_size=2, num_classes=10, embed_dim=[64, 128], depths=[2, 2], num_heads=[[2, 2], [4, 4]],
                              window_size=[[7, 7], [14, 14]], mlp_ratio=[[2.0, 2.0], [2.0, 2.0]], drop_path_rate=0.0).to(DEV).eval()
    calls = []
    hooks = [m.attn.softmax.register_forward_hook(lambda *a: calls.append(1)) for layer in model.layers for m in layer.blocks]
    timing.reset()
    timing.enable(True)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = model(torch.randn(2, 3, 56, 56, device=DEV))
    torch.cuda.synchronize()
    timing.enable(False)
    for h in hooks:
        h.remove()
    s = timing.summary()
    assert not calls and bool(torch.isfinite(y.float()).all())
    assert s["window_attn_fwd"]["launches"] == 2 and s["window_attn_large_fwd"]["launches"] == 2, s


@pytest.mark.parametrize("what", ["fp32", "dropout_training", "switch"])
def test_uncovered_configurations_stay_composed(what):
    """Composed, and equal to the composed branch selected by the switch bit for bit."""
    c = CASES["w14_shifted"]
    m = make_layer(c, attn_drop=0.1 if what == "dropout_training" else 0.0)
    m.train(what == "dropout_training")
    x, gy = case_inputs(c)
    autocast = what != "fp32"
    torch.manual_seed(11)
    if what == "switch":
        with fused_off():
            a, names, calls = run_layer(m, x, gy, autocast=autocast, fused=True)
    else:
        a, names, calls = run_layer(m, x, gy, autocast=autocast, fused=True)
    assert not (LARGE | SMALL) & names and calls == 1, (names, calls)
    torch.manual_seed(11)
    b, _, _ = run_layer(m, x, gy, autocast=autocast, fused=False)            # the composed branch, selected by the switch
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_eval_mode_with_attn_drop_takes_the_fused_path():
    c = CASES["w14_shifted"]
    m = make_layer(c, attn_drop=0.1).eval()
    x, gy = case_inputs(c)
    _, names, calls = run_layer(m, x, gy, autocast=True, fused=True)
    assert LARGE <= names and calls == 0, names


def test_evaluate_agrees_on_both_paths():
    """A synthetic loader of two batches; the targets are the fp32 model's own top-1 for every other sample and a fixed class
    for the rest, so neither accuracy is trivially 0 or 100."""
    from test_s3 import build
    from cream_amd import s3, timing
    model = build().to(DEV)
    g = torch.Generator().manual_seed(77)
    images = [torch.randn(4, 3, 56, 56, generator=g) for _ in range(2)]
    with torch.no_grad():
        top = [model(x.to(DEV)).float().topk(5, dim=1).indices.cpu() for x in images]
    targets = [torch.where(torch.arange(4) % 2 == 0, t[:, 0], t[:, 3]) for t in top]
    loader = list(zip(images, targets))
    timing.reset()
    timing.enable(True)
    fused = s3.evaluate(model, loader, DEV)
    timing.enable(False)
    assert LARGE & set(timing.summary()) == {"window_attn_large_fwd"}
    with fused_off():
        comp = s3.evaluate(model, loader, DEV)
    print(f"[s3 evaluate] fused {fused}  composed {comp}")
    assert fused["acc1"] == comp["acc1"] == 50.0 and fused["acc5"] == comp["acc5"] == 100.0
    assert abs(fused["loss"] - comp["loss"]) <= 2.0 ** -7 * abs(comp["loss"])
    assert not model.training
