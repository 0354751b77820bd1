"""tests/cga_ref.py checked against itself, without a device: the derived bound passes the kernel's rounding model on every case
and every head, and catches every injected fault on at least one case — so the GPU test that uses it can fail."""
import pytest
import torch

import cga_ref
from cga_ref import CASES, FAULTS

_MADE = {}


def case(tag):
    """(x, ops, the rounding model's output): made once per case and shared, never modified."""
    if tag not in _MADE:
        x, ops = cga_ref.make_case(CASES[tag], seed=sorted(CASES).index(tag))
        _MADE[tag] = (x, ops, cga_ref.kernel_model(x, ops, CASES[tag]["w"]))
    return _MADE[tag]


def test_the_reference_is_the_models_own_forward():
    """`head_reference`, head by head with exact sums in between, is `CascadedGroupAttention.forward` up to `proj` in fp64."""
    from cream_amd import efficientvit
    c = CASES["w7_h2_c48_2x2"]
    x, ops, _ = case("w7_h2_c48_2x2")
    w, h, Cg = c["w"], c["h"], c["Cg"]
    m = efficientvit.CascadedGroupAttention(h * Cg, 16, h, attn_ratio=Cg / 16, resolution=w, kernels=list(c["ks"])).eval()
    efficientvit.replace_batchnorm(m)
    m.double()
    with torch.no_grad():
        for i in range(h):
            m.qkvs[i].weight.copy_(ops["W"][i][:, :, None, None])
            m.qkvs[i].bias.copy_(ops["b"][i])
            m.dws[i].weight.copy_(ops["taps"][i][:, None])
            m.dws[i].bias.copy_(ops["tb"][i])
        m.ab = ops["ab"].double()
        m.proj = torch.nn.Identity()
        xw = cga_ref.partition(x.double(), w).transpose(1, 2).reshape(-1, h * Cg, w, w)
        want = m(xw).flatten(2).transpose(1, 2)                                      # (windows, N, C)
    feat, got = None, []
    for i in range(h):
        xi = x.double()[..., i * Cg:(i + 1) * Cg]
        feat = cga_ref.head_reference(xi if feat is None else feat + xi, i, ops, w)
        got.append(feat)
    got = cga_ref.partition(torch.cat(got, -1), w)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("tag", list(CASES))
def test_bound_passes_the_rounding_model(tag):
    x, ops, out = case(tag)
    res = cga_ref.check_heads(out, x, ops, CASES[tag]["w"])
    for i, ratio, err in res:
        print(f"[cga model {tag}] head {i}: worst error {err:.3e}, worst error / bound {ratio:.3f}")
    assert len(res) == CASES[tag]["h"] and all(ratio <= 1.0 for _, ratio, _ in res), res


def test_bound_is_not_slack():
    """The bound is within a small factor of errors the rounding model really makes: a bound ten times wider would pass
    anything."""
    worst = max(ratio for tag in CASES for _, ratio, _ in cga_ref.check_heads(case(tag)[2], case(tag)[0], case(tag)[1], CASES[tag]["w"]))
    print(f"[cga model] worst error / bound over all cases {worst:.3f}")
    assert worst >= 0.1


@pytest.mark.parametrize("fault", FAULTS)
def test_bound_catches_the_fault(fault):
    caught = []
    for tag, c in CASES.items():
        x, ops, _ = case(tag)
        res = cga_ref.check_heads(cga_ref.kernel_model(x, ops, c["w"], fault=fault), x, ops, c["w"])
        if any(ratio > 1.0 for _, ratio, _ in res):
            caught.append((tag, max(ratio for _, ratio, _ in res)))
    print(f"[cga fault {fault}] caught on {caught}")
    assert caught, fault
