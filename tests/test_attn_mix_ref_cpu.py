"""The method of tests/attn_mix_ref.py, proven without a GPU:
A. the hand-written arithmetic without roundings equals the fp64 autograd reference (so the bound, which is computed from its
   intermediates, is a bound around the reference),
B. with the kernels' bf16 roundings it stays inside the bound at every element of every tensor of every case,
C. the references are the composed branches of cream_amd.miniswin / cream_amd.minivit (fp64), shift != mask_shift included,
D. each deliberate error applied to the reference breaks the bound somewhere on the case list,
E. the case lists cover what they claim."""
import pytest
import torch

import attn_mix_ref as R
from helpers import max_rel


def test_case_lists_cover_what_they_claim():
    W, M = R.WINDOW_CASES, R.MINI_CASES
    assert len(set(W)) == len(W) and len(set(M)) == len(M)
    size = [c for c in W if c.group == "size"]
    assert {c.w for c in size} == set(range(1, 9)) and {R.nt_of(c) for c in size} == {1, 2}
    assert all((c.Hs, c.Ws, c.shift, c.ms) == (2 * c.w, 3 * c.w, c.w // 2, c.w // 2) for c in size)
    assert {(c.H, c.mixed) for c in size} == {(3, True), (5, False)}
    heads = [c for c in W if c.group == "heads"]
    assert {R.hpw_of(c) for c in heads if c.mixed} == {1, 2, 3, 4} and {c.H for c in heads if not c.mixed} == {1, 4, 5, 8, 9, 32}
    assert {c.H for c in heads if c.mixed} == {1, 4, 5, 8, 9, 12, 13, 16}
    for w in (7, 4):
        got = {(c.shift, c.ms) for c in W if c.group == "shift" and c.w == w}
        assert got == {(0, 0), (1, 1), (w - 1, w - 1), (0, w // 2), (w // 2, 0), (2, w - 2)}
    assert {(c.Hs, c.Ws, c.shift, c.ms, c.B) for c in W if c.group == "single"} == {(7, 7, 0, 3, 3), (7, 7, 3, 3, 3)}
    assert [c.scale for c in W if c.group == "scale"] == [32 ** -0.5]
    assert all(c.scale == 0.25 for c in W if c.group != "scale") and all(c.scale == 0.125 for c in M)
    assert {c.H for c in M if c.group == "heads"} == {1, 4, 5, 8, 9, 12}
    assert {(c.H, c.L) for c in M if c.group == "length"} == {(H, L) for H in (5, 12) for L in (1, 2, 31, 32, 33, 63, 64, 65, 197)}
    assert {(c.H, c.L, c.rpe, c.skip) for c in M if c.group == "rpe"} == {
        (H, L, kind, skip) for H, L, skip in ((5, 36, 0), (9, 37, 1), (4, 196, 0), (12, 197, 1)) for kind in ("shared", "perhead")}


def _check(tag, ref, bound, plain, model):
    worst = {}
    for n in ref:
        scale = float(ref[n].abs().max()) + 1e-300
        # A: fp64 noise only (d bl is zero in exact arithmetic: on the scale of d Wl)
        if n == "dbl":
            scale = float(ref["dWl"].abs().max())
        assert float((plain[n] - ref[n]).abs().max()) <= 1e-9 * scale, (n, float((plain[n] - ref[n]).abs().max()), scale)
        assert bound[n].shape == ref[n].shape and bool((bound[n] > 0).all()), n
        worst[n] = R.worst_ratio(model[n], ref[n], bound[n])
    print(f"[attn_mix cpu {tag}] " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    return worst


@pytest.mark.parametrize("case", R.WINDOW_CASES, ids=R.wid)
def test_window_rounding_model_lies_inside_the_bound(case):
    o = R.window_operands(case)
    ref, bound = R.window_ref_and_bound(case)
    _check(R.wid(case), ref, bound, R.window_model(o, rounded=False), R.window_model(o, rounded=True))


@pytest.mark.parametrize("case", R.MINI_CASES, ids=R.mid)
def test_mini_rounding_model_lies_inside_the_bound(case):
    o = R.mini_operands(case)
    ref, bound = R.mini_ref_and_bound(case)
    _check(R.mid(case), ref, bound, R.mini_model(o, rounded=False), R.mini_model(o, rounded=True))


def test_a_store_bound_of_two_to_the_minus_nine_times_ref_is_not_a_bound():
    """Why the store term is half an ulp: one round-to-nearest bf16 conversion is off by up to 2^-8 |x| at the bottom of a
    binade."""
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    err = (R.bf16(x) - x).abs()
    assert float(err) > 2.0 ** -9 * float(x) and float(err) <= float(R.hu(x))
    assert float(R.hu(torch.tensor([1.0], dtype=torch.float64))) == 2.0 ** -8           # 2^-8 |x| at the bottom of the binade
    assert float(R.hu(torch.tensor([1.999], dtype=torch.float64))) == 2.0 ** -8         # 2^-9 |x| at its top


# ---- C: the references against the modules' composed branches ---------------------------------------------------------------
def _window_layer(o):
    """One repeat of a block's attention half in fp64, proj and the norms as identities: the module's own composed branch on
    the case's qkv."""
    from cream_amd import miniswin
    c = o.case
    blk = miniswin.SwinTransformerBlock(c.H * 32, (c.Hs, c.Ws), c.H, window_size=c.w, shift_size=c.ms, drop_path=[0.],
                                        qk_scale=c.scale, is_transform_heads=c.mixed).double()
    assert blk.window_size == c.w and blk.shift_size == c.ms
    with torch.no_grad():
        blk.attn.relative_position_bias_table.copy_(o.table.double())
        if c.mixed:
            for p, t in zip((blk.proj_l[0].weight, blk.proj_l[0].bias, blk.proj_w[0].weight, blk.proj_w[0].bias), o.mix):
                p.copy_(t.double())
    return blk


@pytest.mark.parametrize("sel", [("size", 7, 3, 3, True), ("shift", 7, 2, 5, True), ("shift", 4, 2, 0, True), ("size", 6, 3, 3, False)])
def test_window_reference_is_the_modules_composed_branch(sel):
    group, w, shift, ms, mixed = sel
    case = next(c for c in R.WINDOW_CASES if (c.group, c.w, c.shift, c.ms, c.mixed) == sel)
    o = R.window_operands(case)
    c = case
    blk = _window_layer(o)
    B, L, H, N = c.B, c.Hs * c.Ws, c.H, c.w * c.w
    qkv = o.qkv.double().clone().requires_grad_(True)                                  # (B, L, 3, H, 32)
    x = qkv.view(B, c.Hs, c.Ws, 3 * H * 32)
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    from cream_amd import miniswin
    win = miniswin.window_partition(x, c.w).reshape(-1, N, 3 * H * 32)
    blk.attn.proj = torch.nn.Identity()
    y = blk.attn.attend(win, mask=blk.attn_mask, proj_l=blk.proj_l[0] if mixed else None, proj_w=blk.proj_w[0] if mixed else None)
    y = miniswin.window_reverse(y.view(-1, c.w, c.w, H * 32), c.w, c.Hs, c.Ws)
    if shift > 0:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    y = y.reshape(B, L, H, 32)
    (y * o.do).sum().backward()
    ref = R.window_reference(o)
    got = {"out": y.detach(), "dq": qkv.grad[:, :, 0], "dk": qkv.grad[:, :, 1], "dv": qkv.grad[:, :, 2],
           "dT": blk.attn.relative_position_bias_table.grad}
    if mixed:
        got.update({"dWl": blk.proj_l[0].weight.grad, "dWw": blk.proj_w[0].weight.grad, "dbw": blk.proj_w[0].bias.grad})
    for n, t in got.items():
        assert max_rel(t, ref[n]) < 1e-10, (n, max_rel(t, ref[n]))


@pytest.mark.parametrize("sel", [("heads", 5, 33, None), ("rpe", 9, 37, "perhead"), ("rpe", 5, 36, "shared")])
def test_mini_reference_is_the_modules_composed_branch(sel):
    from cream_amd import minivit
    from cream_amd.irpe import get_rpe_config
    group, H, L, kind = sel
    case = next(c for c in R.MINI_CASES if (c.group, c.H, c.L, c.rpe) == sel)
    o = R.mini_operands(case)
    cfg = get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=kind == "shared", skip=case.skip, rpe_on='k') if kind else None
    m = minivit.MiniAttention(H * 64, num_heads=H, qkv_bias=False, qk_scale=case.scale, rpe_config=cfg, repeated_times=1,
                              use_transform=True).double()
    qkv = o.qkv.double().clone().requires_grad_(True)

    class Given(torch.nn.Module):                             # the case's qkv in place of the projection
        def forward(self, x):
            return qkv.view(case.B, L, 3 * H * 64)

    m.qkv, m.proj = Given(), torch.nn.Identity()
    with torch.no_grad():
        m.conv_l.instances[0].weight.copy_(o.wl.double())
        m.conv_w.instances[0].weight.copy_(o.ww.double())
        if kind:
            m.rpe_k.instances[0].lookup_table_weight.copy_(o.rpe.lookup_table_weight.double())
    y = m(torch.zeros(case.B, L, H * 64, dtype=torch.float64)).view(case.B, L, H, 64)
    (y * o.do).sum().backward()
    ref = R.mini_reference(o)
    got = {"out": y.detach(), "dq": qkv.grad[:, :, 0], "dk": qkv.grad[:, :, 1], "dv": qkv.grad[:, :, 2],
           "dWl": m.conv_l.instances[0].weight.grad.view(H, H), "dWw": m.conv_w.instances[0].weight.grad.view(H, H)}
    if kind:
        got["dWk"] = m.rpe_k.instances[0].lookup_table_weight.grad
    for n, t in got.items():
        assert max_rel(t, ref[n]) < 1e-10, (n, max_rel(t, ref[n]))


# ---- D: sensitivity ---------------------------------------------------------------------------------------------------------------
OLD_SEEN = ("out", "dq", "dk", "dv", "dT", "dWl", "dWw", "dbw", "dWk")      # what max_rel <= 2^-7 ever looked at (dq, dk, dv through a GEMM)


def _broken(faulty, ref, bound):
    new = sorted(n for n in ref if R.worst_ratio(faulty[n], ref[n], bound[n]) > 1.0)
    old = sorted(n for n in ref if n in OLD_SEEN and max_rel(faulty[n], ref[n]) > 2.0 ** -7)
    return new, old


@pytest.mark.parametrize("fault", R.WINDOW_FAULTS)
def test_window_deliberate_errors_break_the_bound(fault):
    hits = {}
    for c in R.WINDOW_CASES:
        if c.group == "heads" and c.H > 9:
            continue                                          # the small cases already decide it
        ref, bound = R.window_ref_and_bound(c)
        new, old = _broken(R.window_reference(R.window_operands(c), fault), ref, bound)
        if new or old:
            hits[R.wid(c)] = (new, old)
    n_new, n_old = sum(1 for v in hits.values() if v[0]), sum(1 for v in hits.values() if v[1])
    only_new = [t for t, v in hits.items() if v[0] and not v[1]]
    print(f"[attn_mix sensitivity window {fault}] bound broken on {n_new} cases, max_rel > 2^-7 on {n_old} cases; tensors new "
          f"{sorted({n for v in hits.values() for n in v[0]})} old {sorted({n for v in hits.values() for n in v[1]})}; "
          f"new only: {only_new}")
    assert n_new >= 1, fault


@pytest.mark.parametrize("fault", R.MINI_FAULTS)
def test_mini_deliberate_errors_break_the_bound(fault):
    hits = 0
    for c in R.MINI_CASES:
        if c.L > 65 or c.H < 2:
            continue
        ref, bound = R.mini_ref_and_bound(c)
        new, _ = _broken(R.mini_reference(R.mini_operands(c), fault), ref, bound)
        hits += bool(new)
    assert hits >= 1, fault
