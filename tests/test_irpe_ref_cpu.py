"""The method of tests/irpe_ref.py, proven without a GPU:
A. the fp64 reference is the model code — `RPEAttention`'s composed core and `detr_attention`'s composed path with real
   irpe.iRPE / iRPE_Cross modules in fp64 — for every method in both modes, with a key padding mask and a rectangular map,
B. the hand-written arithmetic without roundings equals the autograd reference on every tensor (so the bound, which is computed
   from its intermediates, is a bound around the reference),
C. with the kernels' bf16 roundings it stays inside the bound at every element of every tensor of every case of both GPU lists,
D. each deliberate error applied to the reference breaks the bound in every case where it can apply,
E. the case lists cover what they claim."""
import copy

import pytest
import torch

import irpe_ref as R
from helpers import max_rel

ALL_CASES = R.BASE_CASES + R.X_CASES


# ---- E ------------------------------------------------------------------------------------------------------------------------------
def test_case_lists_cover_what_they_claim():
    Bc, Xc = R.BASE_CASES, R.X_CASES
    assert len({R.cid(c) for c in ALL_CASES}) == len(ALL_CASES) and len(set(ALL_CASES)) == len(ALL_CASES)
    assert all(c.fam == "base" and c.D == 64 and c.mask is None and c.layout == "packed" and R.row_width_of(c) == 64 for c in Bc)
    assert all(c.L <= 257 for c in ALL_CASES)
    s50 = R.syn(50)
    assert {c.L for c in Bc if c.tag.startswith("len-")} == {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 257}
    assert all((c.tq, c.tk, c.tv, c.H, c.B) == (s50, s50, s50, 3, 2) for c in Bc if c.tag.startswith("len-"))
    at65 = {(c.tq is not None, c.tk is not None, c.tv is not None) for c in Bc if c.L == 65 and not c.drop and not c.causal
            and all(t in (None, s50) for t in (c.tq, c.tk, c.tv))}
    assert len(at65) == 8
    assert {(c.H, c.tk[3]) for c in Bc if c.tag.startswith("heads-")} == {(1, True), (2, True), (5, True), (1, False)}
    assert {c.B for c in Bc if c.tag.startswith("batch-")} == {1, 3}
    assert {(c.tk[1], c.tq is not None) for c in Bc if c.tag.startswith("nb")} == {(nb, f) for nb in (1, 2, 51, 52, 63, 64) for f in (False, True)}
    assert {c.tag for c in Bc if c.tag.startswith("bias-")} == {f"bias-{w}-nb{nb}" for w in ("q", "k", "qk-ctxv") for nb in (51, 52)}
    mods = [c for c in Bc if c.tag.startswith("mod-")]
    assert {c.L for c in mods} == {50, 37, 40} and {c.hw for c in mods} == {None, (5, 8)}
    assert {(c.tk[1], c.tk[2], c.tk[3]) for c in mods if c.hw is None} == {("product", "ctx", True), ("product", "ctx", False), ("euc", "ctx", False),
                                                                          ("quant", "ctx", False), ("cross", "ctx", False), ("cross", "bias", True)}
    assert {(c.drop, c.L) for c in Bc if c.drop and c.tv is not None} == {(p, L) for p in (0.1, 0.5) for L in (33, 129)}
    assert any(c.drop == 0.25 and (c.tq, c.tk, c.tv) == (None, None, None) and not c.causal for c in Bc)
    assert {c.L for c in Bc if c.causal and c.tk is None and not c.drop} == {1, 32, 33, 77, 128, 129}
    assert any(c.causal and c.tk is not None for c in Bc) and any(c.causal and c.drop for c in Bc)
    assert all(c.scale == 0.125 for c in Bc)
    # x family
    assert all(c.fam == "x" for c in Xc)
    geo = lambda D, W, masked: {c.L for c in Xc if c.D == D and R.row_width_of(c) == W and (c.mask is not None) == masked and  # noqa: E731
                                c.tag.startswith("d")}
    full = {1, 31, 32, 33, 64, 65, 128, 129}
    assert geo(32, 64, False) == full and geo(32, 128, False) == full and geo(64, 128, False) == full and geo(64, 64, True) == full
    assert {c.tk[1] for c in Xc if R.row_width_of(c) == 128 and c.D == 32} >= {65, 81, 127, 128}
    for nb in (65, 127, 128):
        assert {c.L for c in Xc if c.tk is not None and c.tk[1] == nb} >= {32, 33, 128, 129}
    assert {c.mask for c in Xc if c.mask} >= set(R.MASKS) - {"none"}
    assert any(c.mask == "tile1" and c.L == 96 for c in Xc)
    assert {c.layout for c in Xc} == {"packed", "separate", "seqfirst"}
    assert any(c.tk is not None and c.tk[2] == "bias" and R.row_width_of(c) == 128 for c in Xc)
    assert {c.H for c in Xc} >= {1, 3, 8}
    assert any(c.drop and c.mask not in (None, "none") for c in Xc) and any(c.causal and c.mask == "last" for c in Xc)
    assert {c.scale for c in Xc if c.D == 32} == {0.25, 32 ** -0.5} and all(c.scale == 0.125 for c in Xc if c.D == 64)
    # nothing the documentation forbids: every image, and under causal every query, keeps a real key (key 0 under causal)
    for c in ALL_CASES:
        ok = R.operands(c).valid()
        assert bool(ok.any(-1).all()), R.cid(c)
        if c.causal:
            assert bool(ok[:, :, :, 0].all()), R.cid(c)


def test_key_masks_are_what_their_names_say():
    L = 65
    m = {k: R.key_mask(k, 2, L) for k in R.MASKS}
    assert all(not bool(t[0].any()) for t in m.values())
    assert m["last"][1].nonzero().flatten().tolist() == [64] and m["from32"][1].nonzero().flatten().tolist() == list(range(32, 65))
    assert R.key_mask("tile1", 2, 96)[1].nonzero().flatten().tolist() == list(range(32, 64))
    assert (~m["allbut0"][1]).nonzero().flatten().tolist() == [0] and (~m["allbutlast"][1]).nonzero().flatten().tolist() == [64]
    assert m["even"][1].nonzero().flatten().tolist() == list(range(1, 65, 2))


# ---- A: the reference against the model code ------------------------------------------------------------------------------------------
def _tie_case(method, mode, path):
    ctx = mode == "ctx"
    t = R.mod(method, mode, perhead=method in ("product", "cross"))
    kw = dict(tq=t, tk=t, tv=t if ctx else R.mod(method, "ctx", True))
    if path == "deit":
        return R.C(f"tie-{method}-{mode}", "base", 37, **kw)                           # 6 x 6 + one skipped token
    return R.C(f"tie-{method}-{mode}", "x", 40, hw=(5, 8), mask="even", **kw)          # rectangular, key padding


def _param_grads(t, grad, L, hw):
    """The table gradient pushed back to the module's own parameters (the cross method's merged table: two of them)."""
    from cream_amd.irpe import iRPE_Cross
    m = copy.deepcopy(t.module).double()
    if type(m) is iRPE_Cross:
        m.merged_table(L, "cpu", *(hw or (None, None))).backward(grad)
        return [p.grad for p in m.parameters()]
    return [grad]


@pytest.mark.parametrize("mode", ["ctx", "bias"])
@pytest.mark.parametrize("method", ["product", "euc", "quant", "cross"])
def test_reference_is_the_model_code(method, mode):
    path = "deit" if (method, mode) in (("product", "ctx"), ("euc", "bias"), ("quant", "ctx"), ("cross", "bias")) else "detr"
    c = _tie_case(method, mode, path)
    o = copy.copy(R.operands(c))
    B, H, L, D = c.B, c.H, c.L, c.D
    mods = [copy.deepcopy(t.module).double() for t in o.terms]
    if method == "cross":                                    # rows + cols summed in fp64, as the fp64 modules add their two gathers
        hw = c.hw or (None, None)
        o.terms = tuple(t._replace(table=m.merged_table(L, "cpu", *hw).detach()) for t, m in zip(o.terms, mods))
    qkv = o.qkv.double().clone().requires_grad_(True)                                  # (B, L, 3, H, D)
    if path == "deit":
        from cream_amd.rpe_attention import RPEAttention
        m = RPEAttention(H * D, num_heads=H, qk_scale=c.scale).double()

        class Given(torch.nn.Module):                                                  # the case's qkv in place of the projection
            weight = bias = None

            def forward(self, x):
                return qkv.view(B, L, 3 * H * D)

        class Through(torch.nn.Identity):
            weight = bias = None

        m.qkv, m.proj = Given(), Through()
        m.rpe_q, m.rpe_k, m.rpe_v = mods
        y = m(torch.zeros(B, L, H * D, dtype=torch.float64)).view(B, L, H, D)
    else:
        from cream_amd.detr_attention import RPEMultiheadAttention
        assert c.scale == float(D) ** -0.5
        m = RPEMultiheadAttention(H * D, H).double()
        m._project = lambda *a: tuple(qkv[:, :, i].permute(1, 0, 2, 3).reshape(L, B, H * D) for i in range(3))
        m.out_proj = torch.nn.Identity()
        m.rpe_q, m.rpe_k, m.rpe_v = mods
        x = torch.zeros(L, B, H * D, dtype=torch.float64)
        y = m(x, x, x, key_padding_mask=o.pad, need_weights=False, hw=c.hw)[0].view(L, B, H, D).permute(1, 0, 2, 3)
    (y * o.dout.double().view(B, L, H, D)).sum().backward()
    ref = R.reference(o)
    perm = lambda t: t.permute(0, 2, 1, 3)                                             # noqa: E731
    got = {"out": perm(y.detach()), "dq": perm(qkv.grad[:, :, 0]), "dk": perm(qkv.grad[:, :, 1]), "dv": perm(qkv.grad[:, :, 2])}
    for n, t in got.items():
        assert max_rel(t, ref[n]) <= 1e-10, (n, max_rel(t, ref[n]))
    for name, t, mm in zip(R.TABLES, o.terms, mods):
        want = _param_grads(t, ref[name], L, c.hw)
        have = [p.grad for p in mm.parameters()]
        assert len(want) == len(have)
        for w, h in zip(want, have):
            assert max_rel(h, w) <= 1e-10, (name, max_rel(h, w))


# ---- B, C ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=R.cid)
def test_rounding_model_lies_inside_the_bound(case):
    o = R.operands(case)
    ref, bound = R.ref_and_bound(case)
    plain, mdl = R.model(o, rounded=False), R.model(o, rounded=True)
    assert set(plain) == set(mdl) == set(ref)
    worst = {}
    for n in ref:
        # B: fp64 noise only.  The absolute 1e-12: with ONE bucket dLK is a row sum of dS — zero in exact arithmetic
        scale = float(ref[n].abs().max())
        assert float((plain[n] - ref[n]).abs().max()) <= 1e-9 * scale + 1e-12, (n, float((plain[n] - ref[n]).abs().max()), scale)
        assert bound[n].shape == ref[n].shape and bool((bound[n] >= 0).all()) and bool(torch.isfinite(bound[n]).all()), n
        worst[n] = R.worst_ratio(mdl[n], ref[n], bound[n])
    print(f"[irpe cpu {R.cid(case)}] " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_the_pin_case_tells_the_two_forms_of_the_key_launch_lookups_apart():
    """rpe_q lookups of the key launch: bf16(s (k Wq)) as in the forward — inside the bound — against bf16(bf16(s k) Wq), which
    for a scale that is no power of two gives the key launch other probabilities than the saved lse belongs to.  On ordinary
    operands the two differ by a rounding, below the bf16 stores; the pin case (irpe_ref.Operands._term) makes k Wq cancel
    exactly, so the second form is off by tenths and dk, dv and the dlq rows leave the bound."""
    case = next(c for c in R.X_CASES if c.tag == "truescale-d32-lq-pin")
    o = R.operands(case)
    ref, bound = R.ref_and_bound(case)
    assert float((o.k @ o.terms[0].table.double()[0]).abs().max()) == 0.0              # exact cancellation, pair by pair
    good, bad = R.model(o), R.model(o, key_lq_scaled_k=True)
    assert all(R.worst_ratio(good[n], ref[n], bound[n]) <= 1.0 for n in ref)
    worst = {n: R.worst_ratio(bad[n], ref[n], bound[n]) for n in ("dk", "dv", "dlq", "dWq")}
    print(f"[irpe pin] key launch on bf16(s k): error / bound " + "  ".join(f"{n} {v:.1f}" for n, v in worst.items()))
    assert all(v > 1.0 for v in worst.values()), worst
    ordinary = next(c for c in R.X_CASES if c.tag == "truescale-d32-qkv49")         # why a pin case is needed at all
    oo = R.operands(ordinary)
    ref, bound = R.ref_and_bound(ordinary)
    bad = R.model(oo, key_lq_scaled_k=True)
    assert all(R.worst_ratio(bad[n], ref[n], bound[n]) <= 1.0 for n in ref)


def test_bound_tightness_per_family():
    """Median of bound / |ref| over the elements of out, dq, dk, dv, per family (printed for the notes): a bound far above the
    2-4e-2 (out, dv) and 1.6e-2 .. 3e-1 (dq, dk) of the window and Mini-DeiT tests would check nothing."""
    for fam, cases in (("base", R.BASE_CASES), ("x", R.X_CASES)):
        med = {}
        for n in ("out", "dq", "dk", "dv"):
            rel = []
            for c in cases:
                ref, bound = R.ref_and_bound(c)
                live = ref[n] != 0
                rel.append((bound[n][live] / ref[n][live].abs()).flatten())
            med[n] = float(torch.cat(rel).median())
        print(f"[irpe tightness {fam}] median bound / |ref|: " + "  ".join(f"{n} {v:.2e}" for n, v in med.items()))
        assert med["out"] <= 4e-2 and med["dv"] <= 4e-2 and med["dq"] <= 3e-1 and med["dk"] <= 3e-1, med


# ---- D: sensitivity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", R.FAULTS)
def test_deliberate_errors_break_the_bound(fault):
    applies = [c for c in ALL_CASES if R.fault_applies(fault, c)]
    assert applies, fault
    missed, seen = [], set()
    for c in applies:
        ref, bound = R.ref_and_bound(c)
        faulty = R.reference(R.operands(c), fault)
        broken = sorted(n for n in ref if not R.worst_ratio(faulty[n], ref[n], bound[n]) <= 1.0)
        seen.update(broken)
        if not broken:
            missed.append(R.cid(c))
    print(f"[irpe sensitivity {fault}] applies to {len(applies)} cases, bound broken on {len(applies) - len(missed)}; tensors {sorted(seen)}; "
          f"missed: {missed}")
    assert not missed, (fault, missed)
