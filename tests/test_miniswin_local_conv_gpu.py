"""Mini-Swin's local convolution on the device through `SwinTransformerBlock` (dim 64, 2 heads, window 7, two repeats,
is_transform_FFN) on a 14 x 14 and a 7 x 7 map, taps and local_norm weights randomised: the timing regions follow the flag;
without autocast fused and composed agree within the fp32 parity bar (1e-3 max-rel); under bf16 autocast the fused route is no
further from the fp32 run than max(2 x composed, 2^-7) per tensor; repeat r reads repeat r's taps only; reruns are
bit-identical."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, C = 3, 64
REGIONS = {"token_dwconv7_fwd", "token_dwconv7_bwd"}


def make_block(res):
    from cream_amd import miniswin
    torch.manual_seed(1234 + res)
    blk = miniswin.SwinTransformerBlock(dim=C, input_resolution=(res, res), num_heads=2, window_size=7, shift_size=3,
                                        drop_path=(0., 0.), is_sep_layernorm=True, is_transform_FFN=True, is_transform_heads=True)
    blk.custom_init_weights()
    for r in range(2):
        nn.init.normal_(blk.local_conv_list[r].weight, 0.0, 0.1)
        nn.init.normal_(blk.local_conv_list[r].bias, 0.0, 0.1)
        nn.init.normal_(blk.local_norm_list[r].weight, 1.0, 0.2)
        nn.init.normal_(blk.local_norm_list[r].bias, 0.0, 0.2)
    return blk.to(DEV)


def tensors_of(blk, y, x):
    out = {"y": y.detach().float(), "dx": x.grad.float()}
    for name in ("local_conv_list", "local_norm_list"):
        for n, p in getattr(blk, name).named_parameters():
            out[f"d {name}.{n}"] = p.grad.float().clone()
    return out


def run_block(blk, res, fused, autocast, regions=None):
    """One forward + backward of the whole block -> {tensor name: fp32 tensor}."""
    from cream_amd import timing
    blk.fused_local_conv = fused
    g = torch.Generator().manual_seed(77 + res)
    x = torch.randn(B, res * res, C, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(B, res * res, C, generator=g).to(DEV)
    blk.zero_grad(set_to_none=True)
    timing.reset()
    timing.enable(True)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = blk(x)
        y.float().backward(dy)
        torch.cuda.synchronize()
    finally:
        timing.enable(False)
    if regions is not None:
        regions.update({k: v["launches"] for k, v in timing.summary().items() if k in REGIONS})
    return tensors_of(blk, y, x)


def max_rel(a, b):
    """max |a - b| / max |b| (the measure of tests/helpers.py), on the device."""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("res", [14, 7])
def test_regions_follow_the_flag(res):
    blk = make_block(res)
    for autocast in (False, True):
        on, off = {}, {}
        run_block(blk, res, True, autocast, on)
        run_block(blk, res, False, autocast, off)
        assert on == {"token_dwconv7_fwd": 2, "token_dwconv7_bwd": 2} and off == {}, (autocast, on, off)


@pytest.mark.parametrize("res", [14, 7])
def test_fp32_fused_against_composed(res):
    blk = make_block(res)
    fused, composed = run_block(blk, res, True, False), run_block(blk, res, False, False)
    assert set(fused) == set(composed) and len(fused) == 2 + 4 + 4
    worst = {k: max_rel(fused[k], composed[k]) for k in fused}
    print(f"[miniswin local conv {res}x{res} fp32] max-rel fused vs composed: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= 1e-3 for v in worst.values()), worst


@pytest.mark.parametrize("res", [14, 7])
def test_autocast_fused_no_further_from_fp32_than_composed(res):
    blk = make_block(res)
    ref = run_block(blk, res, False, False)
    fused, composed = run_block(blk, res, True, True), run_block(blk, res, False, True)
    bad = {}
    for k in ref:
        ef, ec = max_rel(fused[k], ref[k]), max_rel(composed[k], ref[k])
        print(f"[miniswin local conv {res}x{res} autocast] {k}: fused {ef:.3e}  composed {ec:.3e}")
        if ef > max(2 * ec, 2.0 ** -7):
            bad[k] = (ef, ec)
    assert not bad, bad


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_repeat_reads_its_own_taps_only(autocast):
    """Zeroing local_conv_list[1] leaves repeat 0's output bit-identical (and changes repeat 1's)."""
    res = 14
    blk = make_block(res)
    blk.fused_local_conv = True
    x = torch.randn(B, res * res, C, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        before = [blk.forward_feature(x, bool(r % 2), r) for r in range(2)]
        other = copy.deepcopy(blk)
        for p in other.local_conv_list[1].parameters():
            p.zero_()
        after = [other.forward_feature(x, bool(r % 2), r) for r in range(2)]
    assert torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_reruns_are_bit_identical(autocast):
    res = 14
    blk = make_block(res)
    a, b = run_block(blk, res, True, autocast), run_block(blk, res, True, autocast)
    assert all(torch.equal(a[k], b[k]) for k in a)
