"""EfficientViT (cream_amd/efficientvit.py) on the GPU:
A. the mirror on the reference-made fixture under bf16 autocast in eval mode, fused against composed, before and after
   `replace_batchnorm`: one `cga_attn_fwd` launch per attention layer, logits within max(twice the composed bf16 run's error,
   2^-7) of the fp32 fixture,
B. what stays composed: training mode, a gradient required, fp32, the padded 160 x 160 model, the switches,
C. the fold follows a `load_state_dict` after `eval()`,
D. training mode on the device reproduces the fixture's training logits on the composed path."""
import os
from contextlib import contextmanager

import pytest
import torch

from helpers import max_rel
from test_efficientvit import PADDED, build, errors, fixture, run_eval, run_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REGION = "cga_attn_fwd"


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


def timed(fn):
    """-> (fn(), launches of the fused kernel during it)."""
    from cream_amd import timing
    timing.reset()
    timing.enable(True)
    try:
        out = fn()
    finally:
        timing.enable(False)
    return out, timing.summary().get(REGION, {}).get("launches", 0)


@pytest.mark.parametrize("fused_bn", [False, True])
def test_fixture_model_fused_against_composed(fused_bn):
    from cream_amd import efficientvit
    model = build().to(DEV).eval()
    if fused_bn:
        efficientvit.replace_batchnorm(model)
    want = fixture()["small|logits_fused_bn" if fused_bn else "small|logits_eval"]
    with attention_fused_off():
        comp, n_comp = timed(lambda: run_eval(model, DEV, autocast=True))
    fus, n_fus = timed(lambda: run_eval(model, DEV, autocast=True))
    assert (n_comp, n_fus) == (0, 3), (n_comp, n_fus)            # one launch per attention layer: depth 1 + 1 + 1
    ec, ef = max_rel(comp.float().cpu(), want), max_rel(fus.float().cpu(), want)
    print(f"[efficientvit gpu bf16 fused_bn={fused_bn}] logits: composed {ec:.3e} fused {ef:.3e} bound {max(2 * ec, 2.0 ** -7):.3e}")
    assert ef <= max(2 * ec, 2.0 ** -7), (ec, ef)
    model.fused_attention = False
    _, n_off = timed(lambda: run_eval(model, DEV, autocast=True))
    assert n_off == 0


def test_what_stays_composed():
    model = build().to(DEV)
    _, n = timed(lambda: run_train(model, DEV, autocast=True))                      # training mode
    assert n == 0
    model.eval()
    x = torch.randn(2, 3, 224, 224, device=DEV)

    def with_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return model(x)
    y, n = timed(with_grad)                                                         # eval mode, but the parameters want gradients
    assert n == 0 and y.requires_grad
    _, n = timed(lambda: run_eval(model, DEV, autocast=False))                      # fp32
    assert n == 0
    for p in model.parameters():
        p.requires_grad_(False)
    _, n = timed(with_grad)                                                         # nothing requires a gradient: fused
    assert n == 3
    padded = build(PADDED).to(DEV)
    y, n = timed(lambda: run_eval(padded, DEV, autocast=True, size=160, tag="padded"))
    # the 10 x 10 map pads to 14 (composed); the 5 x 5 and 3 x 3 maps are single windows of their own size
    assert n == 2 and padded.blocks1[0].mixer.m.resolution == 10
    e = max_rel(y.float().cpu(), fixture()["padded|logits_eval"])
    with attention_fused_off():
        ec = max_rel(run_eval(padded, DEV, autocast=True, size=160, tag="padded").float().cpu(), fixture()["padded|logits_eval"])
    print(f"[efficientvit gpu padded] composed {ec:.3e} fused {e:.3e}")
    assert e <= max(2 * ec, 2.0 ** -7)


def test_eval_mode_fold_follows_a_load_state_dict():
    """New weights loaded AFTER eval() must be seen by the fused path."""
    model = build().to(DEV).eval()
    layer = model.blocks2[3].mixer.m                    # 3 heads of 32 on one 7 x 7 window
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 96, 7, 7, generator=g).bfloat16().float().to(DEV)

    def run(fused, autocast=True):
        def go():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                return layer(x)
        if fused:
            y, n = timed(go)
        else:
            with attention_fused_off():
                y, n = timed(go)
        assert n == int(fused)
        return y.float().cpu()

    y1 = run(True)
    assert torch.equal(y1, run(True))                                # the cached fold computes the same
    sd = {k: v.clone() for k, v in layer.state_dict().items()}
    for k in ("attn.qkvs.1.c.weight", "attn.qkvs.0.bn.bias", "attn.dws.0.c.weight", "attn.dws.2.bn.running_mean"):
        sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g).to(DEV)
    sd["attn.qkvs.2.bn.running_var"] = sd["attn.qkvs.2.bn.running_var"] * 1.5
    layer.load_state_dict(sd)
    assert not layer.training
    y2 = run(True)
    assert not torch.equal(y1, y2)
    ref, comp = run(False, autocast=False), run(False)
    eb, ec = max_rel(comp, ref), max_rel(y2, ref)
    print(f"[efficientvit eval fold] composed bf16 {eb:.3e}  fused {ec:.3e}")
    assert ec <= max(2 * eb, 2.0 ** -7)
    assert max_rel(y1, ref) > 4 * max(2 * eb, 2.0 ** -7)             # the stale fold would have been far outside


def test_training_mode_on_the_device_matches_the_fixture():
    model = build().to(DEV)
    (logits, grads), n = timed(lambda: run_train(model, DEV))
    errs = errors(logits, grads)
    print(f"[efficientvit gpu fp32 train] logits {errs['logits']:.2e} worst figure {max(errs.values()):.2e}")
    assert n == 0 and errs["logits"] <= 1e-3                         # fp32 against fp32, as on the CPU: summation order only
