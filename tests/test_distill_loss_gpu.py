"""The fused relation and hidden-relation losses (cream_amd/minivit_distill.py, csrc/distill_loss.hip) on the GPU:
A. each kernel against the module's own composed path: fp32 composed is the reference, composed under bf16 autocast the
   yardstick of bf16 noise — err(fused) <= max(2 err(composed bf16), 2^-7) for the loss and the input gradient, both errors
   max_rel against fp32 composed on the same bf16-rounded inputs;
B. bit-identical reruns;
C. the reference-made student / teacher pair through `distill_losses` on the fused paths, with the switch, and without grad."""
import os
from contextlib import contextmanager

import pytest
import torch

from helpers import max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = {"relation_loss", "hidden_relation_loss"}


@contextmanager
def fused_off():
    old = os.environ.get("CREAM_IRPE_FUSED")
    os.environ["CREAM_IRPE_FUSED"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CREAM_IRPE_FUSED"]
        else:
            os.environ["CREAM_IRPE_FUSED"] = old


def timed(fn):
    """-> (fn(), regions seen)"""
    from cream_amd import timing
    timing.reset()
    timing.enable(True)
    try:
        out = fn()
    finally:
        timing.enable(False)
    return out, set(timing.summary())


def check_bound(what, ref, comp, fus):
    """ref / comp / fus: {name: tensor}.  Prints the three numbers per tensor, returns the offenders."""
    bad = []
    for k in ref:
        eb, ec = max_rel(comp[k], ref[k]), max_rel(fus[k], ref[k])
        bound = max(2 * eb, 2.0 ** -7)
        print(f"[{what}] {k:12s} composed bf16 {eb:.3e}  fused {ec:.3e}  bound {bound:.3e}")
        if not ec <= bound:
            bad.append((k, eb, ec, bound))
    return bad


# ---- A1. relation kernel ---------------------------------------------------------------------------------------------------------
RELATION = {
    "shifted": dict(B=2, res=(14, 14), shift=3, Cs=64, Ct=96),                  # wrap-around addressing, four windows
    "rect": dict(B=2, res=(14, 21), shift=0, Cs=96, Ct=128),                    # non-square map
    "rect_shifted": dict(B=1, res=(21, 14), shift=3, Cs=64, Ct=96),             # swapped axes show up
    "deep": dict(B=3, res=(7, 7), shift=0, Cs=256, Ct=512),                     # chunked contraction, single window
    "groups": dict(B=2, res=(14, 14), shift=0, Cs=128, Ct=192, Ar=2),           # channel groups, depth 64 / 96
    "mixed_layout": dict(B=2, res=(14, 14), shift=3, Cs=64, Ct=96, student_windows=True),
    "many_items": dict(B=80, res=(14, 14), shift=0, Cs=64, Ct=96),              # 320 windows: more than the persistent grid
    "self": dict(B=2, res=(14, 14), shift=3, Cs=64, Ct=64, same=True),
}
_RELATION_RESULTS = {}


def relation_inputs(c, seed=7):
    g = torch.Generator().manual_seed(seed)
    L = c["res"][0] * c["res"][1]
    s = torch.randn(c["B"], L, 3 * c["Cs"], generator=g).bfloat16()
    t = s.clone() if c.get("same") else torch.randn(c["B"], L, 3 * c["Ct"], generator=g).bfloat16()
    return s.to(DEV), t.to(DEV)


def run_relation(c, s, t, dtype, autocast, fused):
    """-> ({loss, d qkv}, regions).  The student's gradient is taken at the map-order qkv whatever the tap's layout."""
    from cream_amd.minivit_distill import QkvTap, relation_loss
    geom = (*c["res"], 7, c["shift"])
    qkv = s.to(dtype).clone().requires_grad_(True)
    s_tap = QkvTap(qkv, geom)
    if c.get("student_windows"):
        s_tap = s_tap.windows()
    t_tap = QkvTap(t.to(dtype), geom)

    def go():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            loss = relation_loss([s_tap], [t_tap], c.get("Ar", 1))
        loss.backward()
        return loss
    if fused:
        loss, names = timed(go)
    else:
        with fused_off():
            loss, names = timed(go)
    return {"loss": loss.detach().float().cpu().reshape(1), "d qkv": qkv.grad.detach().float().cpu()}, names


def relation_case(tag):
    if tag not in _RELATION_RESULTS:
        c = RELATION[tag]
        s, t = relation_inputs(c)
        ref, na = run_relation(c, s, t, torch.float32, autocast=False, fused=True)          # fp32 qkv: stays composed
        comp, nb = run_relation(c, s, t, torch.bfloat16, autocast=True, fused=False)
        fus, nc = run_relation(c, s, t, torch.bfloat16, autocast=True, fused=True)
        _RELATION_RESULTS[tag] = (ref, comp, fus, na, nb, nc)
    return _RELATION_RESULTS[tag]


@pytest.mark.parametrize("tag", list(RELATION))
def test_relation_fused_against_composed(tag):
    ref, comp, fus, na, nb, nc = relation_case(tag)
    assert not NEW & na and not NEW & nb, (na, nb)
    assert "relation_loss" in nc, nc
    assert torch.isfinite(fus["loss"]).all() and torch.isfinite(fus["d qkv"]).all()
    if tag == "self":
        # teacher = student: softmax(A_s) - softmax(A_t) is exactly zero, the loss is the rows' entropy
        assert float(fus["d qkv"].abs().max()) == 0.0
        assert float(fus["loss"]) > 0.5
        ref, comp, fus = ({"loss": d["loss"]} for d in (ref, comp, fus))
    assert not check_bound(f"relation {tag}", ref, comp, fus)


def test_relation_layouts_agree():
    """The student as a tuple of partitioned windows against the teacher's map tap computes what two map taps do."""
    ref = relation_case("shifted")[0]
    fus = relation_case("mixed_layout")[2]
    comp = relation_case("shifted")[1]
    assert not check_bound("relation mixed_layout vs shifted", ref, comp, fus)


# ---- A2. hidden kernel -----------------------------------------------------------------------------------------------------------
HIDDEN = {
    "tail": dict(B=2, L=196, Cs=64, Ct=96),                                      # four rows in the last 64-row tile
    "single_tile": dict(B=3, L=49, Cs=128, Ct=192),
    "many_tiles": dict(B=1, L=784, Cs=32, Ct=64),                                # 13 x 13 tiles
    "wide": dict(B=1, L=49, Cs=768, Ct=1024),                                    # the last stage's widths
    "bf16_in": dict(B=2, L=196, Cs=64, Ct=96, bf16=True),
    "zero_row": dict(B=2, L=196, Cs=64, Ct=96, zero=(1, 77)),
}


def hidden_inputs(c, seed=9):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(c["B"], c["L"], c["Cs"], generator=g).bfloat16()
    t = torch.randn(c["B"], c["L"], c["Ct"], generator=g).bfloat16()
    if "zero" in c:
        s[c["zero"]] = 0.0
    return s.to(DEV), t.to(DEV)


def run_hidden(c, s, t, dtype, autocast, fused):
    from cream_amd.minivit_distill import hidden_relation_loss
    x = s.to(dtype).clone().requires_grad_(True)

    def go():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            loss = hidden_relation_loss([x], [t.to(dtype)])
        loss.backward()
        return loss
    if fused:
        loss, names = timed(go)
    else:
        with fused_off():
            loss, names = timed(go)
    assert x.grad.dtype == dtype
    return {"loss": loss.detach().float().cpu().reshape(1), "d hidden": x.grad.detach().float().cpu()}, names


@pytest.mark.parametrize("tag", list(HIDDEN))
def test_hidden_fused_against_composed(tag):
    c = HIDDEN[tag]
    s, t = hidden_inputs(c)
    ref, na = run_hidden(c, s, t, torch.float32, autocast=False, fused=False)
    comp, nb = run_hidden(c, s, t, torch.float32, autocast=True, fused=False)
    fus, nc = run_hidden(c, s, t, torch.bfloat16 if c.get("bf16") else torch.float32, autocast=True, fused=True)
    assert not NEW & na and not NEW & nb, (na, nb)
    assert "hidden_relation_loss" in nc, nc
    assert torch.isfinite(fus["loss"]).all() and torch.isfinite(fus["d hidden"]).all()
    if "zero" in c:
        # the all-zero token's gradient is g / 1e-12: compared on its own, the other rows without it
        b, i = c["zero"]
        for d in (ref, comp, fus):
            d["d zero row"] = d["d hidden"][b, i].clone()
            d["d hidden"][b, i] = 0.0
        assert float(fus["d zero row"].abs().max()) > 0.0
    assert not check_bound(f"hidden {tag}", ref, comp, fus)


# ---- B. reruns -------------------------------------------------------------------------------------------------------------------
def test_reruns_are_bit_identical():
    c = RELATION["many_items"]
    s, t = relation_inputs(c)
    a, names = run_relation(c, s, t, torch.bfloat16, autocast=True, fused=True)
    b, _ = run_relation(c, s, t, torch.bfloat16, autocast=True, fused=True)
    assert "relation_loss" in names
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c = HIDDEN["many_tiles"]
    s, t = hidden_inputs(c)
    a, names = run_hidden(c, s, t, torch.float32, autocast=True, fused=True)
    b, _ = run_hidden(c, s, t, torch.float32, autocast=True, fused=True)
    assert "hidden_relation_loss" in names
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- C. the whole step -------------------------------------------------------------------------------------------------------------
WEIGHT = "layers.0.blocks.0.attn.qkv.weight"
_PAIR = {}


def pair():
    if not _PAIR:
        from test_minivit_distill import build_pair
        _PAIR["models"] = build_pair(DEV)
    return _PAIR["models"]


def run_step(autocast, fused, grad=True):
    from test_minivit_distill import config, inputs
    from cream_amd.minivit_distill import distill_losses
    student, teacher = pair()
    x = inputs("distill")[0].to(DEV)
    y = torch.zeros(2, dtype=torch.long, device=DEV)
    student.zero_grad(set_to_none=True)

    def go():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast), torch.set_grad_enabled(grad):
            total, parts = distill_losses(student, teacher, x, y, config(True))
        if grad:
            total.backward()
        return total, parts
    if fused:
        (total, parts), names = timed(go)
    else:
        with fused_off():
            (total, parts), names = timed(go)
    out = {"total": total.detach().float().cpu().reshape(1)}
    out.update({k: v.detach().float().cpu().reshape(1) for k, v in parts.items() if k in ("attn", "hidden")})
    if grad:
        out["d " + WEIGHT] = dict(student.named_parameters())[WEIGHT].grad.detach().float().cpu()
    return out, names


def step_case(key):
    if key not in _PAIR:
        _PAIR[key] = run_step(autocast=key != "fp32", fused=key == "fused")
    return _PAIR[key]


def test_whole_step_takes_the_fused_paths():
    """The reference-made pair through `distill_losses` under bf16 autocast: both loss kernels and the fused attention run; the
    total and the gradient of the first shared qkv weight (it collects the relation loss through the tap and everything else
    through the attention's output) stay within the bound of the fp32 composed step."""
    ref, na = step_case("fp32")
    comp, nb = step_case("composed")
    fus, nc = step_case("fused")
    assert not NEW & na and not NEW & nb, (na, nb)
    assert NEW | {"window_attn_fwd", "window_attn_bwd"} <= nc, nc
    assert not check_bound("distill step", ref, comp, fus)


def test_switch_turns_both_losses_off():
    ref, _ = step_case("fp32")
    comp, names = step_case("composed")
    assert not (NEW | {"window_attn_fwd"}) & names, names
    for k in ("total", "attn", "hidden"):
        assert max_rel(comp[k], ref[k]) < 4e-2, (k, float(comp[k]), float(ref[k]))


def test_no_grad_runs_the_forward_only_launch():
    from cream_amd import _lib, minivit_distill as D
    fus, _ = step_case("fused")
    seen = []
    real = (D.relation_core, D.hidden_core)
    D.relation_core = lambda *a: (seen.append(("relation", a[6] is not None)), real[0](*a))[1]
    D.hidden_core = lambda *a: (seen.append(("hidden", bool(a[3]))), real[1](*a))[1]
    try:
        out, names = run_step(autocast=True, fused=True, grad=False)
    finally:
        D.relation_core, D.hidden_core = real
    assert NEW <= names and seen and not any(flag for _, flag in seen), seen
    assert {k for k, _ in seen} == {"relation", "hidden"}
    for k in ("total", "attn", "hidden"):
        assert max_rel(out[k], fus[k]) < 1e-6, (k, float(out[k]), float(fus[k]))
    assert _lib.load() is not None
