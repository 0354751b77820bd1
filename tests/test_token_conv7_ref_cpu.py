"""The yardstick of tests/test_token_conv7_kernel_gpu.py, checked without a device: the hand-written model of the kernels'
arithmetic stays inside the per-element bound of the fp64 reference on every shared case, and each injected fault leaves it on
every case on which it can be expressed."""
from functools import lru_cache

import pytest

from token_conv7_ref import (CASES, CHUNK, FAULTS, MANY_CASES, OUTPUTS, R0_CASES, TILE, cid, kernel_model, operands, ref_and_bound,
                             tiles, worst_ratio)

# The maps on which a fault changes nothing, per fault — stated, then checked against what the model really does.  Only maps
# without a second token in some axis, except for the ignored tap ring: a tap at distance 3 needs a map 4 tokens long somewhere,
# so the 2 x 2 and 3 x 3 maps of the case list cannot show it.
INEXPRESSIBLE = {
    "taps_transposed": {(1, 1)},                          # only the centre tap is inside the map
    "row_end_read_through": {(1, 1), (1, 4)},             # one row: there is no neighbouring row to read into
    "image_read_through": set(),
    "dx_taps_unflipped": {(1, 1)},
    "last_vector_copied": set(),
    "y_residual_dropped": set(),
    "dx_residual_dropped": set(),
    "outer_ring_ignored": {(1, 1), (3, 1), (2, 2), (3, 3)},
    "halo_off_by_one": set(),
}


@lru_cache(maxsize=None)
def _good(c, bf16_io, bias, r):
    return kernel_model(operands(c), bf16_io, bias, r)


def _ratios(c, bf16_io, bias, r, got):
    ref, bound = ref_and_bound(c, bf16_io, bias, r)
    return {k: worst_ratio(got[k], ref[k], bound[k]) for k in OUTPUTS}


def test_case_list_covers_what_the_issue_asks():
    maps = {(c.Hs, c.Ws) for c in CASES}
    assert maps >= {(1, 1), (1, 4), (3, 1), (2, 2), (3, 3), (4, 7), (7, 7), (6, 8), (5, 9), (15, 9), (9, 17), (14, 14)}
    assert {c.Hs for c in CASES} >= {TILE - 1, TILE, TILE + 1} and {c.Ws for c in CASES} >= {TILE - 1, TILE, TILE + 1}
    widths = {c.C for c in CASES}
    assert widths >= {8, 40, 96, 128, 160, 576, 1024} and {c.B for c in CASES} == {1, 3}
    assert min(widths) < CHUNK and CHUNK in widths and any(C > CHUNK and C % CHUNK for C in widths)
    assert any(C % 64 for C in widths)                      # lanes are channels: a wave with idle lanes
    assert all(c.C % 8 == 0 for c in CASES + MANY_CASES) and len(MANY_CASES) >= 2
    assert all((c.Hs, c.Ws) in maps for c in R0_CASES) and len(R0_CASES) >= 6
    assert all(sum((k.Hs, k.Ws) == m for k in CASES) == 2 for m in maps)
    assert all(tiles(c) > 1 for c in MANY_CASES)


@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_model_of_the_kernels_is_inside_the_bound(bf16_io, bias):
    worst = {k: 0.0 for k in OUTPUTS}
    for c, r in [(c, 1) for c in CASES] + [(c, 0) for c in R0_CASES]:
        for k, v in _ratios(c, bf16_io, bias, r, _good(c, bf16_io, bias, r)).items():
            worst[k] = max(worst[k], v)
    print(f"[token conv7 model {'bf16' if bf16_io else 'fp32'}] worst error / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("bf16_io", [True, False], ids=["bf16", "fp32"])
def test_injected_faults_leave_the_bound(fault, bf16_io):
    """Every case on which the fault changes anything moves some element by more than its bound, and the cases on which it
    changes nothing are exactly the stated maps."""
    unchanged, missed = set(), []
    for c in CASES:
        good, bad = _good(c, bf16_io, True, 1), kernel_model(operands(c), bf16_io, True, 1, fault)
        if all((good[k] == bad[k]).all() for k in OUTPUTS):
            unchanged.add((c.Hs, c.Ws))
        elif max(_ratios(c, bf16_io, True, 1, bad).values()) <= 1.0:
            missed.append(cid(c))
    assert not missed, (fault, missed)                      # a fault that is expressible and not caught
    assert unchanged == INEXPRESSIBLE[fault], (fault, unchanged)
    assert all(min(m) < 2 for m in unchanged) or fault == "outer_ring_ignored"
