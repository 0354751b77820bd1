"""The kernels of csrc/window_attn_mix_large.hip, called directly (`fwd_core` / `bwd_core`), against the fp64 CPU reference of
tests/window_mix_large_ref.py — every element of out, lse, delta, dq, dk, dv, d table, d Wl, d bl, d Ww and d bw under the
per-element bound derived there from the kernels' rounding points.  The case list reaches every window size from 9 to 12 (3 to
5 key tiles), every head-slot count at every window size, full and empty last slots, shift != mask_shift, single-window maps, both scales, and
one case with more work items than a grid on eight CUs has workgroups; tests/test_window_mix_large_ref_cpu.py proves the method
on the CPU."""
import pytest
import torch

import window_mix_large_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_mix_large(c):
    """-> ({name: CPU tensor in the layout of R.window_reference}, timing regions seen)"""
    from cream_amd import timing, window_attn_mix_large as W
    o = R.mix_large_operands(c)
    B, L, H, N = c.B, c.Hs * c.Ws, c.H, c.w * c.w
    qkv, dout, table = o.qkv.to(DEV), o.dout.to(DEV), o.table.to(DEV)
    mix = tuple(t.to(DEV) for t in o.mix)
    timing.reset()
    timing.enable(True)
    try:
        out, lse = W.fwd_core(qkv, c.scale, table, o.geometry, mix)
        dqkv, dtab, dmix, delta = W.bwd_core(dout, qkv, lse, c.scale, table, o.geometry, mix, return_delta=True)
        torch.cuda.synchronize()
    finally:
        timing.enable(False)
    names = set(timing.summary())
    assert out.dtype == torch.bfloat16 and dqkv.dtype == torch.bfloat16
    assert all(t.dtype == torch.float32 for t in (lse, delta, dtab) + tuple(dmix))
    assert lse.shape == delta.shape == (B * (L // N), H, R.np_of(c)) == (B * (L // N), H, W.padded_tokens(c.w))
    got = {"out": out.view(B, L, H, 32), "lse": lse[:, :, :N], "delta": delta[:, :, :N], "dq": dqkv[:, :, 0], "dk": dqkv[:, :, 1],
           "dv": dqkv[:, :, 2], "dT": dtab, "dWl": dmix[0], "dbl": dmix[1], "dWw": dmix[2], "dbw": dmix[3]}
    return {n: t.detach().cpu() for n, t in got.items()}, names


def _compare(tag, got, ref, bound):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = {n: R.worst_ratio(got[n], ref[n], bound[n]) for n in ref}
    print(f"[window_mix_large {tag}] error / bound: " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    bad = {n: v for n, v in worst.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("case", R.MIX_LARGE_CASES, ids=R.xid)
def test_mix_large_window_kernels_against_fp64(case):
    ref, bound = R.mix_large_ref_and_bound(case)
    got, names = run_mix_large(case)
    assert {"window_attn_mix_large_fwd", "window_attn_mix_large_bwd"} <= names, names
    assert not {"window_attn_fwd", "window_attn_bwd", "window_attn_large_fwd", "window_attn_large_bwd"} & names, names
    _compare(R.xid(case), got, ref, bound)


def test_many_items_loop_and_sum_and_repeat_bit_for_bit():
    """80 work items: a second run gives the same bits (the parameter gradients above all).  On the whole chip every item has a
    workgroup of its own, so the same case runs once more with all CUs but eight reserved (cream_cu_reserve, the data-parallel
    driver's knob): then every workgroup walks several items and the caller sums fewer, longer partials."""
    import ctypes
    from cream_amd import _lib
    c = R.MANY_CASE
    lib = _lib.load()
    o = R.mix_large_operands(c)
    keep = tuple(t.to(DEV) for t in o.mix)
    d = _lib.WindowAttnMixLargeDesc()
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = c.B, c.H, c.Hs, c.Ws, c.w, c.shift, c.ms, 32
    d.wl, d.bl, d.ww, d.bw = (t.data_ptr() for t in keep)
    items = c.B * (c.Hs // c.w) * (c.Ws // c.w) * R.nt_of(c)
    ref, bound = R.mix_large_ref_and_bound(c)
    with torch.cuda.device(DEV):
        assert 1 < lib.cream_window_attn_mix_large_blocks(ctypes.byref(d)) <= items
    a, _ = run_mix_large(c)
    _compare(R.xid(c), a, ref, bound)
    b, _ = run_mix_large(c)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    prev = lib.cream_cu_reserve(-1)
    try:
        lib.cream_cu_reserve(10 ** 6)                         # never below one CU per XCD: 8 CUs
        with torch.cuda.device(DEV):
            blocks = lib.cream_window_attn_mix_large_blocks(ctypes.byref(d))
        assert 1 < blocks < items, (blocks, items)            # several items per workgroup
        s, _ = run_mix_large(c)
        s2, _ = run_mix_large(c)
    finally:
        lib.cream_cu_reserve(prev)
    _compare(R.xid(c) + "-8cu", s, ref, bound)                # the partials sum to the reference
    for n in s:
        assert torch.equal(s[n], s2[n]), n


def test_the_sweep_reaches_every_size():
    from cream_amd import window_attn_mix_large as W
    C = R.MIX_LARGE_CASES
    assert (R.MIN_WINDOW, R.MAX_WINDOW, R.MAX_HEADS) == (W.MIN_WINDOW, W.MAX_WINDOW, W.MAX_HEADS)
    assert {c.w for c in C} == set(range(W.MIN_WINDOW, W.MAX_WINDOW + 1))
    assert {(c.w, R.nt_of(c), R.slots_of(c)) for c in C} == {(w, nt, s) for w, nt in ((9, 3), (10, 4), (11, 4), (12, 5))
                                                             for s in (1, 2, 3, 4)}
    assert max(c.H for c in C) == W.MAX_HEADS and min(c.H for c in C) == 1
