"""The yardstick of tests/test_token_conv_kernel_gpu.py, checked without a device: the hand-written model of the kernels'
arithmetic stays inside the per-element bound of the fp64 reference on every shared case, and each injected fault leaves it."""
import pytest

from token_conv_ref import CASES, FAULTS, MANY_CASES, OUTPUTS, cid, kernel_model, operands, ref_and_bound, worst_ratio


def _ratios(c, bf16_io, bias, fault=None):
    ref, bound = ref_and_bound(c, bf16_io, bias)
    got = kernel_model(operands(c), bf16_io, bias, fault)
    return {k: worst_ratio(got[k], ref[k], bound[k]) for k in OUTPUTS}


def test_case_list_covers_what_the_issue_asks():
    assert {(c.Hs, c.Ws) for c in CASES} == {(1, 1), (1, 4), (3, 1), (2, 2), (3, 3), (5, 9), (7, 7), (14, 14)}
    assert {c.C for c in CASES} == {8, 40, 64, 160, 576} and {c.B for c in CASES} == {1, 3}
    assert all(c.C % 8 == 0 for c in CASES + MANY_CASES)
    assert any(c.B * c.Hs * c.Ws > 2048 * 3 for c in MANY_CASES)              # more tokens than one pass of the grid at C = 576


@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_model_of_the_kernels_is_inside_the_bound(bf16_io, bias):
    worst = {k: 0.0 for k in OUTPUTS}
    for c in CASES:
        for k, v in _ratios(c, bf16_io, bias).items():
            worst[k] = max(worst[k], v)
    print(f"[token conv model {'bf16' if bf16_io else 'fp32'}] worst error / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
def test_injected_faults_leave_the_bound(fault, bf16_io):
    """Every case on which the fault changes anything moves some element by more than its bound."""
    changed, caught = [], []
    for c in CASES:
        o = operands(c)
        good, bad = kernel_model(o, bf16_io, True), kernel_model(o, bf16_io, True, fault)
        if all((good[k] == bad[k]).all() for k in OUTPUTS):
            continue                                          # e.g. a 1 x 1 map of one image has no neighbour to misread
        changed.append(cid(c))
        if max(_ratios(c, bf16_io, True, fault).values()) > 1.0:
            caught.append(cid(c))
    assert len(changed) >= 6 and caught == changed, (fault, sorted(set(changed) - set(caught)))
