"""The method of tests/window_mix_large_ref.py, proven without a GPU:
A. the hand-written arithmetic without roundings equals the fp64 autograd reference (so the bound, which is computed from its
   intermediates, is a bound around the reference),
B. with the kernels' bf16 roundings it stays inside the bound at every element of every tensor of every case,
C. each deliberate error of attn_mix_ref.WINDOW_FAULTS applied to the reference breaks the bound somewhere on the case list
   (every case has w >= 9),
D. the case list covers what it claims."""
import pytest

import window_mix_large_ref as R


def test_case_list_covers_what_it_claims():
    C = R.MIX_LARGE_CASES
    assert len(set(C)) == len(C) and R.MANY_CASE not in C
    assert all(c.mixed and R.MIN_WINDOW <= c.w <= R.MAX_WINDOW and 1 <= c.H <= R.MAX_HEADS for c in C + [R.MANY_CASE])
    size = [c for c in C if c.group == "size"]
    assert [c.w for c in size] == [9, 10, 11, 12] and [R.nt_of(c) for c in size] == [3, 4, 4, 5]
    assert [R.np_of(c) - c.w * c.w for c in size] == [15, 28, 7, 16]
    assert all((c.B, c.H, c.Hs, c.Ws, c.shift, c.ms) == (2, 3, 2 * c.w, 3 * c.w, c.w // 2, c.w // 2) for c in size)
    heads = [c for c in C if c.group == "heads"]
    assert [c.H for c in heads] == [1, 4, 5, 8, 9, 13, 16] and all((c.w, c.Hs, c.Ws) == (12, 12, 12) for c in heads)
    assert {R.slots_of(c) for c in heads} == {1, 2, 3, 4} and {c.H % 4 for c in heads} == {0, 1}      # full and empty last slots
    shift = [c for c in C if c.group == "shift"]
    assert {(c.shift, c.ms) for c in shift} == {(0, 0), (1, 1), (11, 11), (0, 6), (6, 0), (2, 10)}
    assert all((c.w, c.Hs, c.Ws, c.H) == (12, 24, 36, 2) for c in shift)
    assert {(c.B, c.Hs, c.Ws, c.w, c.shift, c.ms) for c in C if c.group == "single"} == {(3, 12, 12, 12, 0, 6), (3, 12, 12, 12, 6, 6)}
    assert [c.scale for c in C if c.group == "scale"] == [32 ** -0.5] and all(c.scale == 0.25 for c in C if c.group != "scale")
    assert all(c.B <= 2 for c in C if c.group != "single")
    slots = [c for c in C if c.group == "slots"]
    assert [(c.w, c.H) for c in slots] == [(w, H) for w in (9, 10, 11) for H in (5, 9, 16)]
    assert all((c.B, c.Hs, c.Ws, c.shift, c.ms) == (1, 2 * c.w, 2 * c.w, c.w // 2, c.w // 2) for c in slots)
    # every (w, key-tile count, head-slot count) of the range
    assert {(c.w, R.nt_of(c), R.slots_of(c)) for c in C} == {(w, nt, s) for w, nt in ((9, 3), (10, 4), (11, 4), (12, 5))
                                                             for s in (1, 2, 3, 4)}
    m = R.MANY_CASE
    assert (m.B * (m.Hs // m.w) * (m.Ws // m.w)) * R.nt_of(m) == 80 and m.H == 2


@pytest.mark.parametrize("case", R.MIX_LARGE_CASES, ids=R.xid)
def test_rounding_model_lies_inside_the_bound(case):
    o = R.mix_large_operands(case)
    ref, bound = R.mix_large_ref_and_bound(case)
    plain, model = R.mix_large_model(o, rounded=False), R.mix_large_model(o, rounded=True)
    assert set(plain) == set(ref) == set(bound)
    worst = {}
    for n in ref:
        scale = float(ref[n].abs().max()) + 1e-300
        if n == "dbl":                                        # zero in exact arithmetic (the rows of dS' sum to zero): on the scale of d Wl
            scale = float(ref["dWl"].abs().max())
        assert float((plain[n] - ref[n]).abs().max()) <= 1e-9 * scale, (n, float((plain[n] - ref[n]).abs().max()), scale)   # A
        assert bound[n].shape == ref[n].shape and bool((bound[n] > 0).all()), n
        worst[n] = R.worst_ratio(model[n], ref[n], bound[n])
    print(f"[window_mix_large cpu {R.xid(case)}] " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst                                    # B


@pytest.mark.parametrize("fault", R.WINDOW_FAULTS)
def test_deliberate_errors_break_the_bound(fault):
    hits = {}
    for c in R.MIX_LARGE_CASES:
        if c.H > 5:
            continue                                          # the small cases already decide it
        ref, bound = R.mix_large_ref_and_bound(c)
        faulty = R.window_reference(R.mix_large_operands(c), fault)
        broken = sorted(n for n in ref if R.worst_ratio(faulty[n], ref[n], bound[n]) > 1.0)
        if broken:
            hits[R.xid(c)] = broken
    print(f"[window_mix_large sensitivity {fault}] bound broken on {len(hits)} cases; tensors {sorted({n for v in hits.values() for n in v})}")
    assert hits, fault
