"""csrc/token_dwconv7.hip on the GPU, launch by launch (cream_amd.token_conv.fwd_core7 / bwd_core7): every element of y, dx, dw
and dbias against the fp64 reference of tests/token_conv7_ref.py within its per-element bound, for bf16 and for fp32 I/O, with
and without a bias, with the residual (every case) and without (a subset); cases whose workgroups loop; bit-identical backward
runs; the autograd function; the C ABI's argument checks.  That the bound catches the injected faults is shown without a device
in tests/test_token_conv7_ref_cpu.py."""
import ctypes

import pytest
import torch

from token_conv7_ref import CASES, MANY_CASES, OUTPUTS, R0_CASES, cid, operands, ref_and_bound, tiles, worst_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_kernels(c, bf16_io, bias, r=1):
    from cream_amd import token_conv
    o = operands(c)
    dt = torch.bfloat16 if bf16_io else torch.float32
    x, dy = o.x.to(DEV, dt), o.dy.to(DEV, dt)
    w, b = o.w.to(DEV), (o.bias.to(DEV) if bias else None)
    y = token_conv.fwd_core7(x, w, b, (c.Hs, c.Ws), r)
    dx, dw, db = token_conv.bwd_core7(dy, x, w, (c.Hs, c.Ws), r)
    torch.cuda.synchronize()
    assert y.dtype == dt and dx.dtype == dt and dw.dtype == torch.float32 and db.dtype == torch.float32
    return dict(y=y.cpu(), dx=dx.cpu(), dw=dw.cpu(), db=db.cpu())


def check(c, bf16_io, bias, r=1):
    ref, bound = ref_and_bound(c, bf16_io, bias, r)
    got = run_kernels(c, bf16_io, bias, r)
    ratios = {k: worst_ratio(got[k], ref[k], bound[k]) for k in OUTPUTS}
    print(f"[token conv7 {cid(c)} {'bf16' if bf16_io else 'fp32'} {'bias' if bias else 'nobias'} r={r}] worst error / bound: "
          + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def _blocks(c, bf16_io):
    from cream_amd import _lib
    d = _lib.TokenDwconv7Desc()
    d.B, d.Hs, d.Ws, d.C, d.dtype = c.B, c.Hs, c.Ws, c.C, _lib.BF16 if bf16_io else _lib.F32
    return _lib.load().cream_token_dwconv7_blocks(ctypes.byref(d))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_every_element_within_its_bound(c, bf16_io, bias):
    check(c, bf16_io, bias)


@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("c", R0_CASES, ids=cid)
def test_without_the_residual(c, bf16_io):
    check(c, bf16_io, True, 0)


@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("c", MANY_CASES, ids=cid)
def test_more_tiles_than_workgroups(c, bf16_io):
    blocks = _blocks(c, bf16_io)                           # the tile axis of the forward, dx and gradient launches alike
    assert 1 <= blocks < tiles(c), (blocks, tiles(c))      # every launch loops
    check(c, bf16_io, True)


@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
def test_backward_runs_are_bit_identical(bf16_io):
    for c in (CASES[-1], MANY_CASES[0]):
        a, b = run_kernels(c, bf16_io, False), run_kernels(c, bf16_io, False)
        assert all(torch.equal(a[k], b[k]) for k in OUTPUTS), cid(c)


@pytest.mark.parametrize("io", ["bf16", "fp32", "fp32-autocast"])
def test_autograd_function_and_timing_regions(io):
    """token_dwconv7 under autograd (with a bias and the residual) returns what the launches return, in the dtype of its input
    whether or not bf16 autocast is on — the taps and the bias stay the fp32 parameters — and the regions count bytes from the
    shapes."""
    from cream_amd import timing, token_conv
    c = next(c for c in CASES if (c.Hs, c.Ws, c.C) == (5, 9, 576))
    o = operands(c)
    bf16_io = io == "bf16"
    dt = torch.bfloat16 if bf16_io else torch.float32
    x = o.x.to(DEV, dt).requires_grad_(True)
    w, b = o.w.to(DEV).requires_grad_(True), o.bias.to(DEV).requires_grad_(True)
    timing.reset()
    timing.enable(True)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=io != "fp32"):
            y = token_conv.token_dwconv7(x, w, b, (c.Hs, c.Ws), residual=True)
        y.backward(o.dy.to(DEV, y.dtype))
    finally:
        timing.enable(False)
    s = timing.summary()
    assert y.dtype == dt and x.grad.dtype == dt and w.grad.dtype == torch.float32 and w.grad.shape == o.w.shape
    size, L = (2 if bf16_io else 4), c.Hs * c.Ws
    assert s["token_dwconv7_fwd"]["launches"] == 1 and s["token_dwconv7_bwd"]["launches"] == 1
    assert s["token_dwconv7_fwd"]["bytes"] == token_conv.fwd_bytes7(c.B, L, c.C, size, True) == 2 * c.B * L * c.C * size + 50 * c.C * 4
    blocks = _blocks(c, bf16_io)
    assert s["token_dwconv7_bwd"]["bytes"] == token_conv.bwd_bytes7(c.B, L, c.C, size, blocks) \
        == 4 * c.B * L * c.C * size + 49 * c.C * 4 + blocks * 50 * c.C * 4
    direct = run_kernels(c, bf16_io, True, 1)
    got = dict(y=y.detach().cpu(), dx=x.grad.cpu(), dw=w.grad.cpu(), db=b.grad.cpu())
    assert all(torch.equal(got[k], direct[k]) for k in OUTPUTS)
    ref, bound = ref_and_bound(c, bf16_io, True, 1)
    ratios = {k: worst_ratio(got[k], ref[k], bound[k]) for k in OUTPUTS}
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_cabi_rejects_without_a_launch():
    """C = 60, a misaligned base, a wrong part_blocks and an fp16 dtype come back as error codes; no kernel runs (the outputs
    keep their fill)."""
    from cream_amd import _lib
    lib = _lib.load()
    B, Hs, Ws, C = 2, 5, 6, 64
    x = torch.randn(B * Hs * Ws * C + 8, device=DEV)
    w = torch.randn(C * 49, device=DEV)
    y = torch.full_like(x, 7.0)
    dx = torch.full_like(x, 7.0)

    def desc(**kw):
        d = _lib.TokenDwconv7Desc()
        d.x, d.w, d.y, d.dy, d.dx = x.data_ptr(), w.data_ptr(), y.data_ptr(), x.data_ptr(), dx.data_ptr()
        d.B, d.Hs, d.Ws, d.C, d.dtype, d.residual = B, Hs, Ws, C, _lib.F32, 1
        for k, v in kw.items():
            setattr(d, k, v)
        blocks = lib.cream_token_dwconv7_blocks(ctypes.byref(d))
        part = torch.full((max(blocks, 1), 50 * C), 7.0, device=DEV)
        d.part, d.part_blocks = part.data_ptr(), kw.get("part_blocks", max(blocks, 1))
        return d, part

    def fwd(d):
        return lib.cream_token_dwconv7_fwd(ctypes.byref(d), None)

    def bwd(d):
        return lib.cream_token_dwconv7_bwd(ctypes.byref(d), None)

    parts = []
    for kw, want in ((dict(C=60), -1), (dict(x=x.data_ptr() + 4), -1), (dict(dtype=_lib.F16), -2), (dict(residual=2), -1),
                     (dict(Ws=0), -1)):
        d, part = desc(**kw)
        parts.append(part)
        assert (fwd(d), bwd(d)) == (want, want), (kw, fwd(d), bwd(d))
    for wrong in (10 ** 6, 0):                              # part_blocks is the backward's alone
        d, part = desc(part_blocks=wrong)
        parts.append(part)
        assert bwd(d) == -1, wrong
    assert lib.cream_token_dwconv7_blocks(ctypes.byref(desc(C=60)[0])) == -1
    assert lib.cream_token_dwconv7_blocks(ctypes.byref(desc(dtype=_lib.F16)[0])) == -2
    assert lib.cream_token_dwconv7_part_size(64) == 3200 and lib.cream_token_dwconv7_part_size(60) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((dx == 7.0).all()) and all(bool((p == 7.0).all()) for p in parts)
