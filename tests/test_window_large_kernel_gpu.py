"""The kernels of csrc/window_attn_large.hip, called directly (`fwd_core` / `bwd_core`), against the fp64 CPU reference of
tests/window_large_ref.py — every element of out, lse, delta, dq, dk, dv and d table under the per-element bound derived there
from the kernels' rounding points.  The case list reaches every window size from 9 to 14 (3 to 7 key tiles), 1 / 3 / 5 / 32
heads, shift != mask_shift, single-window maps, both scales, and one case with more windows than the persistent grid has
window lanes; tests/test_window_large_ref_cpu.py proves the method on the CPU."""
import pytest
import torch

import window_large_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_large(c):
    """-> ({name: CPU tensor in the layout of R.window_reference}, timing regions seen)"""
    from cream_amd import timing, window_attn_large
    o = R.large_operands(c)
    B, L, H, N = c.B, c.Hs * c.Ws, c.H, c.w * c.w
    qkv, dout, table = o.qkv.to(DEV), o.dout.to(DEV), o.table.to(DEV)
    timing.reset()
    timing.enable(True)
    try:
        out, lse = window_attn_large.fwd_core(qkv, c.scale, table, o.geometry)
        dqkv, dtab, delta = window_attn_large.bwd_core(dout, qkv, lse, c.scale, table, o.geometry, return_delta=True)
        torch.cuda.synchronize()
    finally:
        timing.enable(False)
    names = set(timing.summary())
    assert out.dtype == torch.bfloat16 and dqkv.dtype == torch.bfloat16 and dtab.dtype == torch.float32
    assert lse.shape == delta.shape == (B * (L // N), H, R.np_of(c)) == (B * (L // N), H, window_attn_large.padded_tokens(c.w))
    got = {"out": out.view(B, L, H, 32), "lse": lse[:, :, :N], "delta": delta[:, :, :N], "dq": dqkv[:, :, 0], "dk": dqkv[:, :, 1],
           "dv": dqkv[:, :, 2], "dT": dtab}
    return {n: t.detach().cpu() for n, t in got.items()}, names


def _compare(tag, got, ref, bound):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = {n: R.worst_ratio(got[n], ref[n], bound[n]) for n in ref}
    print(f"[window_large {tag}] error / bound: " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    bad = {n: v for n, v in worst.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("case", R.LARGE_CASES, ids=R.lid)
def test_large_window_kernels_against_fp64(case):
    ref, bound = R.large_ref_and_bound(case)
    got, names = run_large(case)
    assert {"window_attn_large_fwd", "window_attn_large_bwd"} <= names and not {"window_attn_fwd", "window_attn_bwd"} & names, names
    _compare(R.lid(case), got, ref, bound)


def test_many_items_loop_and_sum_and_repeat_bit_for_bit():
    """160 windows x 2 heads: the caller sums many partials, and a second run gives the same bits (d table above all).  The
    grid has a window lane per (window, head) as long as the chip has room, so the same case runs once more with all CUs but
    eight reserved (cream_cu_reserve, the data-parallel driver's knob): then every workgroup walks several windows."""
    import ctypes
    from cream_amd import _lib
    c = R.MANY_CASE
    lib = _lib.load()
    d = _lib.WindowAttnLargeDesc()
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = c.B, c.H, c.Hs, c.Ws, c.w, c.shift, c.ms, 32
    nwin = c.B * (c.Hs // c.w) * (c.Ws // c.w)
    ref, bound = R.large_ref_and_bound(c)
    with torch.cuda.device(DEV):
        assert 1 < lib.cream_window_attn_large_blocks(ctypes.byref(d)) <= nwin
    a, _ = run_large(c)
    _compare(R.lid(c), a, ref, bound)
    b, _ = run_large(c)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    prev = lib.cream_cu_reserve(-1)
    try:
        lib.cream_cu_reserve(10 ** 6)                         # never below one CU per XCD: 8 CUs
        with torch.cuda.device(DEV):
            lanes = lib.cream_window_attn_large_blocks(ctypes.byref(d))
        assert 1 < lanes < nwin, (lanes, nwin)                # several windows per workgroup
        s, _ = run_large(c)
        s2, _ = run_large(c)
    finally:
        lib.cream_cu_reserve(prev)
    _compare(R.lid(c) + "-8cu", s, ref, bound)
    for n in s:
        assert torch.equal(s[n], s2[n]), n


def test_the_sweep_reaches_every_size():
    from cream_amd import window_attn_large as W
    assert {c.w for c in R.LARGE_CASES} == set(range(W.MIN_WINDOW, W.MAX_WINDOW + 1))
    assert max(c.H for c in R.LARGE_CASES) == W.MAX_HEADS and min(c.H for c in R.LARGE_CASES) == 1
