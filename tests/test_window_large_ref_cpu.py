"""The method of tests/window_large_ref.py, proven without a GPU:
A. the hand-written arithmetic without roundings equals the fp64 autograd reference (so the bound, which is computed from its
   intermediates, is a bound around the reference),
B. with the kernels' bf16 roundings it stays inside the bound at every element of every tensor of every case,
C. each deliberate error applied to the reference breaks the bound somewhere on the case list,
D. the case list covers what it claims."""
import pytest

import window_large_ref as R


def test_case_list_covers_what_it_claims():
    C = R.LARGE_CASES
    assert len(set(C)) == len(C) and R.MANY_CASE not in C
    size = [c for c in C if c.group == "size"]
    assert [c.w for c in size] == [9, 10, 11, 12, 13, 14] and [R.np_of(c) // 32 for c in size] == [3, 4, 4, 5, 6, 7]
    assert 81 - 64 == 17 and 196 - 192 == 4                                              # real keys in the last tile at w = 9, 14
    assert all((c.B, c.Hs, c.Ws, c.shift, c.ms) == (2, 2 * c.w, 3 * c.w, c.w // 2, c.w // 2) for c in size)
    assert {(c.H, c.w) for c in C if c.group == "heads"} == {(1, 14), (3, 14), (5, 14), (32, 14)}
    shift = [c for c in C if c.group == "shift"]
    assert {(c.shift, c.ms) for c in shift} == {(0, 0), (1, 1), (11, 11), (0, 6), (6, 0)}
    assert all(c.w == 12 and c.Hs != c.Ws for c in shift)
    assert {(c.Hs, c.Ws, c.w, c.ms) for c in C if c.group == "single"} == {(14, 14, 14, 0), (14, 14, 14, 7)}
    assert [c.scale for c in C if c.group == "scale"] == [32 ** -0.5] and all(c.scale == 0.25 for c in C if c.group != "scale")
    m = R.MANY_CASE
    assert (m.B, m.Hs, m.Ws, m.w, m.H) == (40, 28, 28, 14, 2)
    assert all(not c.mixed for c in C + [m])


@pytest.mark.parametrize("case", R.LARGE_CASES, ids=R.lid)
def test_rounding_model_lies_inside_the_bound(case):
    o = R.large_operands(case)
    ref, bound = R.large_ref_and_bound(case)
    plain, model = R.large_model(o, rounded=False), R.large_model(o, rounded=True)
    assert set(plain) == set(ref) == set(bound)
    worst = {}
    for n in ref:
        scale = float(ref[n].abs().max()) + 1e-300
        assert float((plain[n] - ref[n]).abs().max()) <= 1e-9 * scale, (n, float((plain[n] - ref[n]).abs().max()), scale)   # A
        assert bound[n].shape == ref[n].shape and bool((bound[n] > 0).all()), n
        worst[n] = R.worst_ratio(model[n], ref[n], bound[n])
    print(f"[window_large cpu {R.lid(case)}] " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst                                    # B


@pytest.mark.parametrize("fault", R.LARGE_FAULTS)
def test_deliberate_errors_break_the_bound(fault):
    hits = {}
    for c in R.LARGE_CASES:
        if c.H > 5:
            continue                                          # the small cases already decide it
        ref, bound = R.large_ref_and_bound(c)
        faulty = R.window_reference(R.large_operands(c), fault)
        broken = sorted(n for n in ref if R.worst_ratio(faulty[n], ref[n], bound[n]) > 1.0)
        if broken:
            hits[R.lid(c)] = broken
    print(f"[window_large sensitivity {fault}] bound broken on {len(hits)} cases; tensors {sorted({n for v in hits.values() for n in v})}")
    assert hits, fault
