"""csrc/token_dwconv.hip on the GPU, launch by launch (cream_amd.token_conv.fwd_core / bwd_core): every element of y, dx, dw
and dbias against the fp64 reference of tests/token_conv_ref.py within its per-element bound, for bf16 and for fp32 I/O, with
and without a bias; cases whose workgroups loop; bit-identical backward runs; the autograd function.  That the bound catches
the injected faults is shown without a device in tests/test_token_conv_ref_cpu.py."""
import pytest
import torch

from token_conv_ref import CASES, MANY_CASES, OUTPUTS, cid, operands, ref_and_bound, worst_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_kernels(c, bf16_io, bias):
    from cream_amd import token_conv
    o = operands(c)
    dt = torch.bfloat16 if bf16_io else torch.float32
    x, dy = o.x.to(DEV, dt), o.dy.to(DEV, dt)
    w, b = o.w.to(DEV), (o.bias.to(DEV) if bias else None)
    y = token_conv.fwd_core(x, w, b, (c.Hs, c.Ws))
    dx, dw, db = token_conv.bwd_core(dy, x, w, (c.Hs, c.Ws))
    torch.cuda.synchronize()
    assert y.dtype == dt and dx.dtype == dt and dw.dtype == torch.float32 and db.dtype == torch.float32
    return dict(y=y.cpu(), dx=dx.cpu(), dw=dw.cpu(), db=db.cpu())


def check(c, bf16_io, bias):
    ref, bound = ref_and_bound(c, bf16_io, bias)
    got = run_kernels(c, bf16_io, bias)
    ratios = {k: worst_ratio(got[k], ref[k], bound[k]) for k in OUTPUTS}
    print(f"[token conv {cid(c)} {'bf16' if bf16_io else 'fp32'} {'bias' if bias else 'nobias'}] worst error / bound: "
          + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_every_element_within_its_bound(c, bf16_io, bias):
    check(c, bf16_io, bias)


@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("c", MANY_CASES, ids=cid)
def test_more_tokens_than_one_pass_of_the_grid(c, bf16_io):
    from cream_amd import _lib
    import ctypes
    d = _lib.TokenDwconv3Desc()
    d.B, d.Hs, d.Ws, d.C, d.dtype = c.B, c.Hs, c.Ws, c.C, _lib.BF16 if bf16_io else _lib.F32
    blocks = _lib.load().cream_token_dwconv3_blocks(ctypes.byref(d))
    vec = 8 if bf16_io else 4
    slots = 256 // min(c.C // vec, 256)
    assert blocks >= 1 and blocks * slots < c.B * c.Hs * c.Ws, (blocks, slots)           # the gradient launch loops
    check(c, bf16_io, True)


@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
def test_backward_runs_are_bit_identical(bf16_io):
    for c in (CASES[-1], MANY_CASES[0]):
        a, b = run_kernels(c, bf16_io, False), run_kernels(c, bf16_io, False)
        assert all(torch.equal(a[k], b[k]) for k in OUTPUTS), cid(c)


@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
def test_autograd_function_and_timing_regions(bf16_io):
    """token_dwconv3 under autograd (with a bias, under autocast for bf16) returns what the launches return, and the regions
    count bytes from the shapes."""
    from cream_amd import timing, token_conv
    c = next(c for c in CASES if (c.Hs, c.Ws, c.C) == (5, 9, 576))
    o = operands(c)
    x = o.x.to(DEV).requires_grad_(True)
    w, b = o.w.to(DEV).requires_grad_(True), o.bias.to(DEV).requires_grad_(True)
    timing.reset()
    timing.enable(True)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16_io):
            y = token_conv.token_dwconv3(x, w, b, (c.Hs, c.Ws))
        y.backward(o.dy.to(DEV, y.dtype))
    finally:
        timing.enable(False)
    s = timing.summary()
    assert y.dtype == (torch.bfloat16 if bf16_io else torch.float32)
    size = 2 if bf16_io else 4
    assert s["token_dwconv3_fwd"]["launches"] == 1 and s["token_dwconv3_bwd"]["launches"] == 1
    assert s["token_dwconv3_fwd"]["bytes"] == token_conv.fwd_bytes(c.B, c.Hs * c.Ws, c.C, size, True)
    ref, bound = ref_and_bound(c, bf16_io, True)
    got = dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad)
    assert x.grad.dtype == torch.float32 and w.grad.shape == o.w.shape
    if bf16_io:                                                                 # x.grad went through the cast's backward: exact
        assert torch.equal(x.grad, x.grad.bfloat16().float())
    ratios = {k: worst_ratio(got[k].cpu(), ref[k], bound[k]) for k in OUTPUTS}
    assert all(v <= 1.0 for v in ratios.values()), ratios
