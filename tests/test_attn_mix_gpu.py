"""The kernels of csrc/window_attn.hip and csrc/mini_attn.hip, called directly (`fwd_core` / `bwd_core`), against the fp64 CPU
references of tests/attn_mix_ref.py — every element of every returned tensor (out, lse, delta, dq, dk, dv and the parameter
gradients) under the per-element bound derived there from the kernels' rounding points.  The case lists reach every window
size from 1 to 8 (both key-tile counts), every head-slot instantiation, shift != mask_shift, single-window maps and the
lengths around the 32-token tiles; tests/test_attn_mix_ref_cpu.py proves the method on the CPU."""
import copy

import pytest
import torch

import attn_mix_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _timed(fn):
    from cream_amd import timing
    timing.reset()
    timing.enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        timing.enable(False)
    return res, set(timing.summary())


def run_window(c):
    """-> ({name: CPU tensor in the layout of R.window_reference}, timing regions seen)"""
    from cream_amd import window_attn
    o = R.window_operands(c)
    B, L, H, N = c.B, c.Hs * c.Ws, c.H, c.w * c.w
    qkv, dout, table = o.qkv.to(DEV), o.dout.to(DEV), o.table.to(DEV)
    mix = None if o.mix is None else tuple(t.to(DEV) for t in o.mix)

    def go():
        out, lse = window_attn.fwd_core(qkv, c.scale, table, o.geometry, mix)
        return (out, lse) + window_attn.bwd_core(dout, qkv, lse, c.scale, table, o.geometry, mix, return_delta=True)

    (out, lse, dqkv, dtab, dmix, delta), names = _timed(go)
    assert out.dtype == torch.bfloat16 and dqkv.dtype == torch.bfloat16 and lse.shape == delta.shape == (B * (L // N), H, 64)
    got = {"out": out.view(B, L, H, 32), "lse": lse[:, :, :N], "delta": delta[:, :, :N], "dq": dqkv[:, :, 0], "dk": dqkv[:, :, 1],
           "dv": dqkv[:, :, 2], "dT": dtab}
    if mix is not None:
        got.update({"dWl": dmix[0], "dbl": dmix[1], "dWw": dmix[2], "dbw": dmix[3]})
    else:
        assert dmix is None
    return {n: t.detach().cpu() for n, t in got.items()}, names


def run_mini(c):
    from cream_amd import irpe_fused, mini_attn
    o = R.mini_operands(c)
    B, L, H = c.B, c.L, c.H
    qkv, dout, wl, ww = o.qkv.to(DEV), o.dout.to(DEV), o.wl.to(DEV), o.ww.to(DEV)
    rpe = copy.deepcopy(o.rpe).to(DEV) if o.rpe is not None else None
    term = irpe_fused._term(rpe, L, DEV)

    def go():
        out, lse = mini_attn.fwd_core(qkv, c.scale, term, wl, ww)
        return (out, lse) + mini_attn.bwd_core(dout, qkv, lse, c.scale, term, wl, ww, return_delta=True)

    (out, lse, dqkv, dtab, dwl, dww, delta), names = _timed(go)
    assert out.dtype == torch.bfloat16 and lse.shape == (B, H, L) and (dtab is None) == (rpe is None)
    got = {"out": out.view(B, L, H, 64), "lse": lse, "delta": delta[:, :, :L], "dq": dqkv[:, :, 0], "dk": dqkv[:, :, 1],
           "dv": dqkv[:, :, 2], "dWl": dwl.view(H, H), "dWw": dww.view(H, H)}
    if dtab is not None:
        got["dWk"] = dtab
    return {n: t.detach().cpu() for n, t in got.items()}, names


def _compare(tag, got, ref, bound):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = {n: R.worst_ratio(got[n], ref[n], bound[n]) for n in ref}
    print(f"[attn_mix {tag}] error / bound: " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    bad = {n: v for n, v in worst.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("case", R.WINDOW_CASES, ids=R.wid)
def test_window_kernels_against_fp64(case):
    ref, bound = R.window_ref_and_bound(case)
    got, names = run_window(case)
    assert {"window_attn_fwd", "window_attn_bwd"} <= names, names
    _compare(R.wid(case), got, ref, bound)


@pytest.mark.parametrize("case", R.MINI_CASES, ids=R.mid)
def test_mini_kernels_against_fp64(case):
    ref, bound = R.mini_ref_and_bound(case)
    got, names = run_mini(case)
    assert {"mini_attn_fwd", "mini_attn_bwd"} <= names, names
    _compare(R.mid(case), got, ref, bound)


def test_the_sweeps_reach_every_instantiation():
    """From H and w alone: both key-tile counts, all four head-slot counts of the mixed window kernels and the plain one,
    all three of mini_attn — and every one of those cases is in the lists the two tests above run."""
    from cream_amd import mini_attn, window_attn
    size = [c for c in R.WINDOW_CASES if c.group == "size"]
    assert {R.nt_of(c) for c in size if c.mixed} == {1, 2} and {R.nt_of(c) for c in size if not c.mixed} == {1, 2}
    assert {c.w for c in size if R.nt_of(c) == 1} == {1, 2, 3, 4, 5} and {c.w for c in size if R.nt_of(c) == 2} == {6, 7, 8}
    heads = [c for c in R.WINDOW_CASES if c.group == "heads"]
    assert {R.hpw_of(c) for c in heads if c.mixed} == {1, 2, 3, 4}
    assert max(c.H for c in heads if c.mixed) == window_attn.MAX_HEADS_MIXED and max(c.H for c in heads) == window_attn.MAX_HEADS
    assert {(c.H + 3) // 4 for c in R.MINI_CASES} == {1, 2, 3} and max(c.H for c in R.MINI_CASES) == mini_attn.MAX_HEADS
    assert all(c.w * c.w <= window_attn.MAX_WINDOW_TOKENS for c in R.WINDOW_CASES)


def _pick_window(**kw):
    return next(c for c in R.WINDOW_CASES if all(getattr(c, k) == v for k, v in kw.items()))


@pytest.mark.parametrize("which", ["w4", "w8", "mixed12", "mini_H5_L33"])
def test_reruns_are_bit_identical(which):
    if which == "mini_H5_L33":
        case = next(c for c in R.MINI_CASES if (c.group, c.H, c.L) == ("heads", 5, 33))
        a, _ = run_mini(case)
        b, _ = run_mini(case)
    else:
        case = {"w4": _pick_window(group="size", w=4, mixed=True), "w8": _pick_window(group="size", w=8, mixed=True),
                "mixed12": _pick_window(group="heads", H=12, mixed=True)}[which]
        a, _ = run_window(case)
        b, _ = run_window(case)
    for n in a:
        assert torch.equal(a[n], b[n]), n
