"""The kernels of csrc/window_attn_xl.hip, called directly (`fwd_core` / `bwd_core`), against the fp64 CPU reference of
tests/window_xl_ref.py — every element of out, lse, delta, dq, dk, dv and d table under the per-element bound derived there
from the kernels' rounding points.  The case list reaches windows of 15, 16, 17, 24, 31 and 32 (8 to 32 key tiles, with 31, 0 and
1 .. padded or real keys in the last one), 1 / 2 / 3 / 32 heads, non-square maps of several windows, both scales, and one case
with more work items than the persistent grid has lanes; tests/test_window_xl_ref_cpu.py proves the method on the CPU."""
import pytest
import torch

import window_xl_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
XL = {"window_attn_xl_fwd", "window_attn_xl_bwd"}
OTHERS = {"window_attn_fwd", "window_attn_bwd", "window_attn_large_fwd", "window_attn_large_bwd"}


def run_xl(c):
    """-> ({name: CPU tensor in the layout of R.xl_reference}, timing regions seen)"""
    from cream_amd import timing, window_attn_xl
    o = R.xl_operands(c)
    B, L, H, N = c.B, c.Hs * c.Ws, c.H, c.w * c.w
    qkv, dout, table = o.qkv.to(DEV), o.dout.to(DEV), o.table.to(DEV)
    timing.reset()
    timing.enable(True)
    try:
        out, lse = window_attn_xl.fwd_core(qkv, c.scale, table, o.geometry)
        dqkv, dtab, delta = window_attn_xl.bwd_core(dout, qkv, lse, c.scale, table, o.geometry, return_delta=True)
        torch.cuda.synchronize()
    finally:
        timing.enable(False)
    names = set(timing.summary())
    assert out.dtype == torch.bfloat16 and dqkv.dtype == torch.bfloat16 and dtab.dtype == torch.float32
    assert lse.shape == delta.shape == (B * (L // N), H, R.np_of(c)) == (B * (L // N), H, window_attn_xl.padded_tokens(c.w))
    got = {"out": out.view(B, L, H, 32), "lse": lse[:, :, :N], "delta": delta[:, :, :N], "dq": dqkv[:, :, 0], "dk": dqkv[:, :, 1],
           "dv": dqkv[:, :, 2], "dT": dtab}
    return {n: t.detach().cpu() for n, t in got.items()}, names


def _compare(tag, got, ref, bound):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = {n: R.worst_ratio(got[n], ref[n], bound[n]) for n in ref}
    print(f"[window_xl {tag}] error / bound: " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    bad = {n: v for n, v in worst.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("case", R.XL_CASES, ids=R.xid)
def test_xl_window_kernels_against_fp64(case):
    ref, bound = R.xl_ref_and_bound(case)
    got, names = run_xl(case)
    assert XL <= names and not OTHERS & names, names
    _compare(R.xid(case), got, ref, bound)


def test_many_items_loop_and_sum_and_repeat_bit_for_bit():
    """36 windows x 2 query blocks x 2 heads: the caller sums many partials, and a second run gives the same bits (d table
    above all).  The grid has a lane per work item as long as the chip has room, so the same case runs once more with all CUs
    but eight reserved (cream_cu_reserve, the data-parallel driver's knob): then every workgroup walks several items."""
    import ctypes
    from cream_amd import _lib
    c = R.MANY_CASE
    lib = _lib.load()
    d = _lib.WindowAttnXlDesc()
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = c.B, c.H, c.Hs, c.Ws, c.w, 0, 0, 32
    nitems = c.B * (c.Hs // c.w) * (c.Ws // c.w) * ((R.np_of(c) // 32 + 3) // 4)
    ref, bound = R.xl_ref_and_bound(c)
    with torch.cuda.device(DEV):
        assert 1 < lib.cream_window_attn_xl_blocks(ctypes.byref(d)) <= nitems
    a, _ = run_xl(c)
    _compare(R.xid(c), a, ref, bound)
    b, _ = run_xl(c)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    prev = lib.cream_cu_reserve(-1)
    try:
        lib.cream_cu_reserve(10 ** 6)                         # never below one CU per XCD: 8 CUs
        with torch.cuda.device(DEV):
            lanes = lib.cream_window_attn_xl_blocks(ctypes.byref(d))
        assert 1 < lanes < nitems, (lanes, nitems)            # several items per workgroup
        s, _ = run_xl(c)
        s2, _ = run_xl(c)
    finally:
        lib.cream_cu_reserve(prev)
    _compare(R.xid(c) + "-8cu", s, ref, bound)
    for n in s:
        assert torch.equal(s[n], s2[n]), n


def test_the_sweep_reaches_both_ends():
    from cream_amd import window_attn_xl as W
    ws = {c.w for c in R.XL_CASES}
    assert min(ws) == W.MIN_WINDOW == 15 and max(ws) == W.MAX_WINDOW == 32
    assert max(c.H for c in R.XL_CASES) == W.MAX_HEADS == 32 and min(c.H for c in R.XL_CASES) == 1
