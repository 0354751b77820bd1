"""TinyViT (cream_amd/tinyvit.py) on the GPU, on the fused window attentions and the token-layout depthwise convolution:
A. one block against its own composed branches (fp32 composed as the reference, bf16 composed as the yardstick of bf16 noise),
B. the mirror on the reference-made fixture, on the fused paths: no composed attention and no `Conv2d` of a block runs,
C. the BatchNorm running statistics of the fused convolution against the composed one,
D. the eval-mode fold follows a `load_state_dict` after `eval()`."""
import os
from contextlib import contextmanager

import pytest
import torch

from helpers import max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LARGE = {"window_attn_large_fwd", "window_attn_large_bwd"}
SMALL = {"window_attn_fwd", "window_attn_bwd"}
CONV = {"token_dwconv3_fwd", "token_dwconv3_bwd"}


@contextmanager
def attention_fused_off():
    old = os.environ.get("CREAM_IRPE_FUSED")
    os.environ["CREAM_IRPE_FUSED"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CREAM_IRPE_FUSED"]
        else:
            os.environ["CREAM_IRPE_FUSED"] = old


@contextmanager
def composed(blocks):
    """Both routings off: CREAM_IRPE_FUSED=0 and fused_local_conv=False on the same code."""
    old = [b.fused_local_conv for b in blocks]
    for b in blocks:
        b.fused_local_conv = False
    try:
        with attention_fused_off():
            yield
    finally:
        for b, f in zip(blocks, old):
            b.fused_local_conv = f


def make_block(c, seed=0):
    from cream_amd import tinyvit
    torch.manual_seed(seed)
    blk = tinyvit.TinyViTBlock(c["H"] * 32, c["res"], c["H"], window_size=c["window"], mlp_ratio=2.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        blk.attn.attention_biases.copy_(0.3 * torch.randn(blk.attn.attention_biases.shape, generator=g))
        blk.attn.qkv.bias.copy_(0.1 * torch.randn(blk.attn.qkv.bias.shape, generator=g))
        blk.local_conv.bn.weight.copy_(1.0 + 0.1 * torch.randn(blk.dim, generator=g))
        blk.local_conv.bn.bias.copy_(0.1 * torch.randn(blk.dim, generator=g))
        blk.local_conv.bn.running_mean.copy_(0.1 * torch.randn(blk.dim, generator=g))
        blk.local_conv.bn.running_var.copy_(0.5 + torch.rand(blk.dim, generator=g))
    return blk.to(DEV)


def run_block(blk, x, gy, autocast, fused, train=True):
    """-> ({name: tensor}, regions seen, softmax calls of the composed attention, calls of the block's Conv2d)"""
    from cream_amd import timing
    from contextlib import nullcontext
    blk.train(train)
    blk.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    calls = {"softmax": 0, "conv": 0}
    hooks = [blk.attn.softmax.register_forward_hook(lambda *a: calls.__setitem__("softmax", calls["softmax"] + 1)),
             blk.local_conv.c.register_forward_hook(lambda *a: calls.__setitem__("conv", calls["conv"] + 1))]
    timing.reset()
    timing.enable(True)
    try:
        with (nullcontext() if fused else composed([blk])), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = blk(x)
        (y.float() * gy).sum().backward()
    finally:
        timing.enable(False)
        for h in hooks:
            h.remove()
    res = {"out": y, "dx": x.grad, "d qkv.weight": blk.attn.qkv.weight.grad, "d attention_biases": blk.attn.attention_biases.grad,
           "d local_conv.c.weight": blk.local_conv.c.weight.grad, "d bn.weight": blk.local_conv.bn.weight.grad}
    return {k: v.detach().float().cpu() for k, v in res.items()}, set(timing.summary()), calls["softmax"], calls["conv"]


CASES = {
    "w7": dict(H=2, res=(28, 28), window=7, B=2, regions=SMALL),                # 16 windows of 7 x 7: window_attn
    "w14_single": dict(H=3, res=(14, 14), window=14, B=3, regions=LARGE),       # the map is one 14 x 14 window
    "w12_rect": dict(H=2, res=(24, 36), window=12, B=1, regions=LARGE),         # the 384 model's window on a non-square map
}


def case_inputs(c, seed=5):
    g = torch.Generator().manual_seed(seed)
    E, L = c["H"] * 32, c["res"][0] * c["res"][1]
    x = torch.randn(c["B"], L, E, generator=g).bfloat16().float().to(DEV)          # the same bf16-rounded input for all
    gy = torch.randn(c["B"], L, E, generator=g).to(DEV)
    return x, gy


@pytest.mark.parametrize("tag", list(CASES))
def test_fused_against_composed(tag):
    """err(fused) <= max(2 err(composed bf16), 2^-7) for out, dx, d qkv.weight, d attention_biases, d local_conv.c.weight and
    d bn.weight, both against the fp32 composed path; the regions and the hooks say which code ran."""
    c = CASES[tag]
    blk = make_block(c)
    x, gy = case_inputs(c)
    ref, names_a, soft_a, conv_a = run_block(blk, x, gy, autocast=False, fused=False)
    comp, names_b, soft_b, conv_b = run_block(blk, x, gy, autocast=True, fused=False)
    fus, names_c, soft_c, conv_c = run_block(blk, x, gy, autocast=True, fused=True)
    assert not (LARGE | SMALL | CONV) & (names_a | names_b) and (soft_a, soft_b, conv_a, conv_b) == (1, 1, 1, 1), (names_a, names_b)
    assert c["regions"] | CONV <= names_c and not ((LARGE | SMALL) - c["regions"]) & names_c and (soft_c, conv_c) == (0, 0), names_c
    bad = []
    for k in ref:
        eb, ec = max_rel(comp[k], ref[k]), max_rel(fus[k], ref[k])
        bound = max(2 * eb, 2.0 ** -7)
        print(f"[tinyvit block {tag}] {k:22s} composed bf16 {eb:.3e}  fused {ec:.3e}  bound {bound:.3e}")
        if not ec <= bound:
            bad.append((k, eb, ec))
    assert not bad, bad


def test_fp32_on_a_device_keeps_the_attention_composed_and_runs_the_convolution_in_fp32():
    c = CASES["w7"]
    blk = make_block(c)
    x, gy = case_inputs(c)
    ref, _, _, _ = run_block(blk, x, gy, autocast=False, fused=False)
    got, names, soft, conv = run_block(blk, x, gy, autocast=False, fused=True)
    assert CONV <= names and not (LARGE | SMALL) & names and (soft, conv) == (1, 0), names
    worst = {k: max_rel(got[k], ref[k]) for k in ref}
    print(f"[tinyvit block fp32 conv] worst {max(worst.values()):.2e}")
    assert max(worst.values()) <= 1e-4, worst                    # fp32 against fp32: summation order only


@pytest.mark.parametrize("what", ["switch", "padded", "w24"])
def test_uncovered_attention_stays_composed(what):
    from cream_amd import tinyvit
    if what == "switch":
        blk, B = make_block(CASES["w7"]), 2
    elif what == "padded":
        blk, B = make_block(dict(H=2, res=(20, 20), window=7)), 2
    else:
        blk, B = tinyvit.TinyViTBlock(64, (24, 24), 2, window_size=24).to(DEV), 1
    L = blk.input_resolution[0] * blk.input_resolution[1]
    g = torch.Generator().manual_seed(3)
    x, gy = torch.randn(B, L, 64, generator=g).to(DEV), torch.randn(B, L, 64, generator=g).to(DEV)
    if what == "switch":
        with attention_fused_off():
            _, names, soft, conv = run_block(blk, x, gy, autocast=True, fused=True)
    else:
        _, names, soft, conv = run_block(blk, x, gy, autocast=True, fused=True)
    assert not (LARGE | SMALL) & names and soft == 1, (names, soft)
    assert CONV <= names and conv == 0                           # the switch means the attention only; the convolution is covered


def test_running_statistics_of_the_fused_convolution():
    """The same block, attention composed in both runs, so BatchNorm's input differs only by the convolution's routing: bf16
    values that differ by at most one bf16 ulp (2^-8 relative).  The batch mean moves by at most 2^-8 of the mean magnitude, the
    variance by twice that, and a running statistic takes momentum = 0.1 of it: 0.2 * 2^-8 of the largest statistic."""
    c = CASES["w7"]
    x, gy = case_inputs(c)
    stats = []
    for fused_conv in (False, True):
        blk = make_block(c)
        blk.fused_local_conv = fused_conv
        with attention_fused_off():
            _, names, _, conv = run_block(blk, x, gy, autocast=True, fused=True)
        assert (CONV <= names) == fused_conv and conv == (0 if fused_conv else 1)
        bn = blk.local_conv.bn
        stats.append((bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)))
    (m0, v0, n0), (m1, v1, n1) = stats
    em, ev = max_rel(m1.cpu(), m0.cpu()), max_rel(v1.cpu(), v0.cpu())
    print(f"[tinyvit bn stats] running_mean {em:.2e}  running_var {ev:.2e}  bound {0.2 * 2.0 ** -8:.2e}")
    assert n0 == n1 == 1 and em <= 0.2 * 2.0 ** -8 and ev <= 0.2 * 2.0 ** -8


def test_whole_model_on_fixture_takes_the_fused_paths():
    """Every block of the fixture model is covered (2 heads with window 7, 3 heads with window 14): no composed attention and
    no `Conv2d` of a block may run.  The logits stay within max(twice the composed bf16 run's error, 2^-7) of the
    reference-made fixture, the gradient figures as a set likewise, the running statistics within 2^-7 of the composed bf16
    run's."""
    from test_tinyvit import build, errors, run_train
    from cream_amd import timing
    blocks = lambda m: [b for layer in m.layers[1:] for b in layer.blocks]          # noqa: E731
    model_c = build().to(DEV)
    with composed(blocks(model_c)):
        logits_c, grads_c = run_train(model_c, DEV, autocast=True)
    model = build().to(DEV)
    calls = []
    hooks = [h for b in blocks(model) for h in (b.attn.softmax.register_forward_hook(lambda *a: calls.append("softmax")),
                                                b.local_conv.c.register_forward_hook(lambda *a: calls.append("conv")))]
    timing.reset()
    timing.enable(True)
    logits_f, grads_f = run_train(model, DEV, autocast=True)
    timing.enable(False)
    for h in hooks:
        h.remove()
    s = timing.summary()
    assert not calls and SMALL | LARGE | CONV <= set(s), (calls, set(s))
    for name, n in (("window_attn_fwd", 2), ("window_attn_bwd", 2), ("window_attn_large_fwd", 2), ("window_attn_large_bwd", 2),
                    ("token_dwconv3_fwd", 4), ("token_dwconv3_bwd", 4)):
        assert s[name]["launches"] == n, (name, s[name])
    ec, ef = errors(logits_c, grads_c), errors(logits_f, grads_f)
    print(f"[tinyvit gpu bf16] logits: composed {ec['logits']:.3e} fused {ef['logits']:.3e}; worst gradient figure: composed "
          f"{max(v for k, v in ec.items() if k != 'logits'):.2e} fused {max(v for k, v in ef.items() if k != 'logits'):.2e}")
    assert ef["logits"] <= max(2 * ec["logits"], 2.0 ** -7), (ec["logits"], ef["logits"])
    # the gradients: 202 scalar figures (norm and strided sample per parameter), each one draw of bf16 noise on either path —
    # measured, the fused figure is the larger one in 100 to 105 of them, and a different handful exceeds twice its composed
    # counterpart in every run.  The yardstick is therefore applied to the figures as a set: their root mean square and their
    # maximum, each within max(twice the composed run's, 2^-7).
    gc, gf = [v for k, v in ec.items() if k != "logits"], [v for k, v in ef.items() if k != "logits"]
    rms = lambda v: (sum(t * t for t in v) / len(v)) ** 0.5          # noqa: E731
    print(f"[tinyvit gpu bf16] gradient figures: rms composed {rms(gc):.3e} fused {rms(gf):.3e}; max composed {max(gc):.3e} fused {max(gf):.3e}")
    assert len(gf) == len(gc) >= 200
    assert rms(gf) <= max(2 * rms(gc), 2.0 ** -7) and max(gf) <= max(2 * max(gc), 2.0 ** -7)
    sd_c, sd_f = model_c.state_dict(), model.state_dict()
    worst = 0.0
    for k in sd_f:
        if k.endswith(("running_mean", "running_var")):
            worst = max(worst, max_rel(sd_f[k].cpu(), sd_c[k].cpu()))
        elif k.endswith("num_batches_tracked"):
            assert int(sd_f[k]) == int(sd_c[k]) == 1, k
    print(f"[tinyvit gpu bf16] running statistics, fused against composed: worst {worst:.2e}")
    assert worst <= 2.0 ** -7


def test_eval_mode_fold_follows_a_load_state_dict():
    """eval(): BatchNorm folded into taps and bias, one launch, no Conv2d.  New weights loaded AFTER eval() must be seen."""
    from cream_amd import timing
    c = CASES["w14_single"]
    blk = make_block(c).eval()
    x, _ = case_inputs(c)

    def run(fused, autocast=True):
        calls = []
        h = blk.local_conv.c.register_forward_hook(lambda *a: calls.append(1))
        timing.reset()
        timing.enable(True)
        try:
            with torch.no_grad(), (composed([blk]) if not fused else attention_fused_off()), \
                    torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = blk(x)
        finally:
            timing.enable(False)
            h.remove()
        s = timing.summary()
        return y.float().cpu(), s.get("token_dwconv3_fwd", {}).get("launches", 0), len(calls)

    y1, launches, calls = run(True)
    assert (launches, calls) == (1, 0)
    y1b, _, _ = run(True)
    assert torch.equal(y1, y1b)                                   # the cached fold computes the same
    g = torch.Generator().manual_seed(9)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    for k in ("local_conv.c.weight", "local_conv.bn.weight", "local_conv.bn.bias", "local_conv.bn.running_mean"):
        sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g).to(DEV)
    sd["local_conv.bn.running_var"] = sd["local_conv.bn.running_var"] * 1.5
    blk.load_state_dict(sd)
    assert not blk.training
    y2, launches, calls = run(True)
    assert (launches, calls) == (1, 0) and not torch.equal(y1, y2)
    ref, _, calls_r = run(False, autocast=False)
    comp, _, calls_c = run(False)
    assert calls_r == calls_c == 1
    eb, ec = max_rel(comp, ref), max_rel(y2, ref)
    print(f"[tinyvit eval fold] composed bf16 {eb:.3e}  fused {ec:.3e}")
    assert ec <= max(2 * eb, 2.0 ** -7)
    assert max_rel(y1, ref) > 4 * max(2 * eb, 2.0 ** -7)          # the stale fold would have been far outside
