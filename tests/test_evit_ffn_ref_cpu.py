"""The depthwise 3 x 3 + FFN kernel's reference, rounding model and bound (tests/evit_ffn_ref.py) and the host side
(cream_amd/evit_ffn.py) without a device: the rounding model stays within the bound of the fp64 reference on every case, every
injected fault leaves it on every case it changes, the C ABI's checks return their codes without a launch, the `usable_*` truth
tables, and the fold against `Conv2d_BN.fuse()`."""
import ctypes

import pytest
import torch

import evit_ffn_ref as R
from evit_ffn_ref import CASES, FAULTS, PW_CASES

_CASE = {}


def case(tag):
    """(x, ops, reference, bound, rounding model): computed once per case and left unchanged."""
    if tag not in _CASE:
        x, ops = R.make_case(CASES[tag], seed=sorted(CASES).index(tag))
        _CASE[tag] = (x, ops, R.reference(x, ops), R.bound(x, ops), R.kernel_model(x, ops))
    return _CASE[tag]


@pytest.mark.parametrize("tag", list(CASES))
def test_rounding_model_stays_within_the_bound(tag):
    x, ops, ref, bnd, out = case(tag)
    c = CASES[tag]
    assert tuple(out.shape) == (c["B"], c["H"], c["W"], c["C"]) and out.dtype == torch.bfloat16
    ratio, err = R.worst(out, ref, bnd)
    print(f"[evit dwffn model {tag}] worst error {err:.3e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_leaves_the_bound_where_it_changes_the_output(fault):
    changed = []
    for tag in CASES:
        x, ops, ref, bnd, good = case(tag)
        bad = R.kernel_model(x, ops, fault=fault)
        if torch.equal(bad.view(torch.int16), good.view(torch.int16)):
            continue
        changed.append(tag)
        ratio, _ = R.worst(bad, ref, bnd)
        assert ratio > 1.0, (fault, tag, ratio)
    print(f"[evit dwffn fault {fault}] changes {changed}")
    assert changed, fault
    if fault == "k_tail_read_through":                   # only the widths that are no multiple of 32 have a tail
        assert set(changed) == {t for t, c in CASES.items() if c["C"] % 32}
    if fault == "halo_wraps_image":                      # a single image has no neighbour to read
        assert set(changed) == {t for t, c in CASES.items() if c["B"] > 1}
    if fault == "taps_transposed":                       # the centre tap is its own transpose
        assert set(changed) == set(CASES) - {"e_c16_1x1"}
    if fault in ("halo_wraps_row", "residual_from_x", "no_relu"):
        assert set(changed) == set(CASES), changed


@pytest.mark.parametrize("tag", list(PW_CASES))
def test_pw_rounding_model_stays_within_the_bound(tag):
    a, res, ops = R.make_pw_case(PW_CASES[tag], seed=sorted(PW_CASES).index(tag))
    ratio, err = R.worst(R.pw_kernel_model(a, res, ops), R.pw_reference(a, res, ops), R.pw_bound(a, res, ops))
    print(f"[evit pw model {tag}] worst error {err:.3e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    # a residual that is dropped, or a bias added twice, leaves the bound
    ops2 = dict(ops, b=2 * ops["b"])
    assert R.worst(R.pw_kernel_model(a, res, ops2), R.pw_reference(a, res, ops), R.pw_bound(a, res, ops))[0] > 1.0
    assert R.worst(R.pw_kernel_model(a, torch.zeros_like(res), ops), R.pw_reference(a, res, ops), R.pw_bound(a, res, ops))[0] > 1.0


def test_layouts_hold_the_same_values():
    c = CASES["g_c32_3x5"]
    xs = [R.make_case(c, seed=3, layout=l)[0] for l in R.LAYOUTS]
    assert all(torch.equal(x, xs[0]) for x in xs)
    # a channels-last NCHW tensor seen as (B, H, W, C) has a token tensor's strides: that is why it goes in without a copy
    assert xs[0].is_contiguous() and not xs[1].is_contiguous() and xs[2].is_contiguous()
    assert all(x.stride(3) == 1 and not any(s % 8 for s in x.stride()[:3]) for x in xs)
    assert float(xs[1]._base[:, -1].float().min()) == R.PAD_VALUE                 # the buffer's padding is not zero


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
BAD_ARG, TOO_LARGE, CHANNEL_STRIDE, BAD_STRIDE, BAD_SHAPE = -1, -4, -5, -6, -7


def _dw_desc(**kw):
    from cream_amd import _lib
    d = _lib.EvitDwffnDesc()
    d.x, d.taps, d.dwb, d.w1, d.b1, d.w2, d.b2, d.out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000
    d.B, d.H, d.W, d.C, d.Ch = 2, 14, 14, 144, 288
    d.xsb, d.xsy, d.xsx, d.xsc = 14 * 14 * 144, 14 * 144, 144, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _pw_desc(**kw):
    from cream_amd import _lib
    d = _lib.EvitPwDesc()
    d.a, d.res, d.w, d.b, d.out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    d.B, d.H, d.W, d.Cin, d.Cout = 2, 7, 7, 96, 64
    d.asb, d.asy, d.asx, d.asc = 7 * 7 * 96, 7 * 96, 96, 1
    d.rsb, d.rsy, d.rsx, d.rsc = 7 * 7 * 64, 7 * 64, 64, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_c_abi_checks_return_their_codes_without_a_launch():
    from cream_amd import _lib
    lib = _lib.load()
    chk, fwd = lib.cream_evit_dwffn_check, lib.cream_evit_dwffn_fwd
    assert chk(ctypes.byref(_dw_desc())) == 0 and chk(None) == BAD_ARG and fwd(None, None) == BAD_ARG
    table = [
        (BAD_SHAPE, [dict(C=8), dict(C=0), dict(C=40), dict(C=400), dict(Ch=16), dict(Ch=48), dict(Ch=800), dict(Ch=0), dict(B=0),
                     dict(H=0), dict(W=0), dict(W=-3)]),
        (TOO_LARGE, [dict(B=1 << 20, H=64, W=64)]),
        (BAD_ARG, [dict(x=None), dict(taps=None), dict(dwb=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None),
                   dict(out=None), dict(x=0x1008), dict(w1=0x4002), dict(w2=0x6004), dict(out=0x8008), dict(taps=0x2004),
                   dict(b2=0x7008)]),
        (CHANNEL_STRIDE, [dict(xsc=2), dict(xsc=0), dict(xsc=14 * 14)]),
        (BAD_STRIDE, [dict(xsx=148), dict(xsx=136), dict(xsy=14 * 144 + 4), dict(xsb=-8), dict(xsb=14 * 14 * 144 + 2)]),
    ]
    for code, rows in table:
        for bad in rows:
            assert chk(ctypes.byref(_dw_desc(**bad))) == code and fwd(ctypes.byref(_dw_desc(**bad)), None) == code, (code, bad)
    # what is covered: every published width, the padded recipes' maps, a slice's strides
    for C in (16, 64, 128, 144, 192, 224, 240, 256, 288, 320, 384):
        assert chk(ctypes.byref(_dw_desc(C=C, Ch=2 * C, xsx=C + 8, xsy=17 * (C + 8), xsb=16 * 17 * (C + 8)))) == 0, C
    assert chk(ctypes.byref(_dw_desc(H=1, W=1))) == 0 and chk(ctypes.byref(_dw_desc(H=3, W=5, Ch=32))) == 0
    # the order of the checks: the shape first, then the pointers, then the strides
    assert chk(ctypes.byref(_dw_desc(C=8, x=None, xsc=2))) == BAD_SHAPE and chk(ctypes.byref(_dw_desc(x=None, xsc=2))) == BAD_ARG
    assert chk(ctypes.byref(_dw_desc(xsc=2, xsx=4))) == CHANNEL_STRIDE

    chk, fwd = lib.cream_evit_pw_residual_check, lib.cream_evit_pw_residual_fwd
    assert chk(ctypes.byref(_pw_desc())) == 0 and chk(None) == BAD_ARG and fwd(None, None) == BAD_ARG
    table = [
        (BAD_SHAPE, [dict(Cin=8), dict(Cin=100), dict(Cin=400), dict(Cout=0), dict(Cout=72), dict(Cout=512), dict(B=0), dict(H=0),
                     dict(W=-1)]),
        (TOO_LARGE, [dict(B=1 << 20, H=64, W=64)]),
        (BAD_ARG, [dict(a=None), dict(res=None), dict(w=None), dict(b=None), dict(out=None), dict(a=0x1002), dict(res=0x2008),
                   dict(w=0x3004), dict(b=0x4004), dict(out=0x5008)]),
        (CHANNEL_STRIDE, [dict(asc=7), dict(rsc=49), dict(rsc=0)]),
        (BAD_STRIDE, [dict(asx=100), dict(asx=88), dict(rsx=56), dict(rsy=7 * 64 + 1), dict(asb=-16)]),
    ]
    for code, rows in table:
        for bad in rows:
            assert chk(ctypes.byref(_pw_desc(**bad))) == code and fwd(ctypes.byref(_pw_desc(**bad)), None) == code, (code, bad)
    for Cin, Cout in ((64, 64), (144, 144), (384, 384), (96, 64), (16, 384)):
        assert chk(ctypes.byref(_pw_desc(Cin=Cin, Cout=Cout, asx=Cin, asy=7 * Cin, asb=49 * Cin, rsx=Cout, rsy=7 * Cout,
                                          rsb=49 * Cout))) == 0


# ---- the path decision and the fold -------------------------------------------------------------------------------------------------
def test_usable_truth_tables():
    from cream_amd import evit_ffn
    ok, okp = evit_ffn.usable_dwffn, evit_ffn.usable_pw
    bf, dev = torch.bfloat16, "cuda:0"
    assert evit_ffn.EXCLUDED == frozenset()
    for C in (64, 128, 144, 192, 224, 240, 256, 288, 320, 384):                  # every published width, on every map
        for H in (14, 7, 4, 10, 5, 3):
            assert ok(bf, dev, C, 2 * C, H, H), (C, H)
    assert ok(bf, dev, 16, 32, 1, 1) and ok(bf, dev, 32, 64, 3, 5) and ok(bf, dev, 384, 768, 1, 200) and ok(bf, dev, 64, 32, 7, 7)
    assert not ok(torch.float32, dev, 64, 128, 14, 14) and not ok(torch.float16, dev, 64, 128, 14, 14)
    assert not ok(bf, "cpu", 64, 128, 14, 14)
    assert not ok(bf, dev, 8, 32, 7, 7) and not ok(bf, dev, 72, 160, 7, 7) and not ok(bf, dev, 400, 768, 7, 7)
    assert not ok(bf, dev, 64, 16, 7, 7) and not ok(bf, dev, 64, 48, 7, 7) and not ok(bf, dev, 384, 800, 7, 7)
    assert not ok(bf, dev, 64, 128, 0, 7) and not ok(bf, dev, 64, 128, 7, 0)
    for Cin, Cout in ((64, 64), (144, 144), (384, 384), (96, 64), (16, 384)):
        assert okp(bf, dev, Cin, Cout)
    assert not okp(torch.float32, dev, 64, 64) and not okp(bf, "cpu", 64, 64)
    assert not okp(bf, dev, 8, 64) and not okp(bf, dev, 64, 72) and not okp(bf, dev, 400, 64) and not okp(bf, dev, 64, 448)


def _pair(C=48, seed=0):
    """A `Residual`(depthwise `Conv2d_BN`) and a `Residual`(`FFN`) with every BatchNorm away from its initial state."""
    from cream_amd import efficientvit as ev
    torch.manual_seed(seed)
    dw = ev.Residual(ev.Conv2d_BN(C, C, 3, 1, 1, groups=C))
    ffn = ev.Residual(ev.FFN(C, 2 * C, 7))
    with torch.no_grad():
        for m in list(dw.modules()) + list(ffn.modules()):
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.2)
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    return dw.eval(), ffn.eval()


def _close(a, b, tol=1e-6):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_fold_equals_fuse_on_both_module_forms_and_follows_a_load_state_dict():
    from cream_amd import efficientvit as ev, evit_ffn
    dw, ffn = _pair()
    C, Ch = 48, 96
    p = evit_ffn.fold_dwffn(dw, ffn)
    assert (p["C"], p["Ch"]) == (C, Ch) and evit_ffn.fold_dwffn(dw, ffn) is p and evit_ffn.fold_dwffn(dw.m, ffn.m) is p
    assert tuple(p["taps"].shape) == (9, C) and p["taps"].dtype == torch.float32 and p["taps"].is_contiguous()
    assert tuple(p["w1"].shape) == (Ch, 64) and p["w1"].dtype == torch.bfloat16 and not p["w1"][:, C:].any()
    assert tuple(p["w2"].shape) == (C, Ch) and p["w2"].dtype == torch.bfloat16
    fd, f1, f2 = dw.m.fuse(), ffn.m.pw1.fuse(), ffn.m.pw2.fuse()

    def same_as_fuse(p):
        assert _close(p["taps"], fd.weight[:, 0].reshape(C, 9).t()) and _close(p["dwb"], fd.bias)
        assert torch.equal(p["w1"][:, :C], f1.weight[:, :, 0, 0].bfloat16()) or _close(p["w1"][:, :C].float(), f1.weight[:, :, 0, 0], 2.0 ** -8)
        assert _close(p["w2"].float(), f2.weight[:, :, 0, 0], 2.0 ** -8)
        assert _close(p["b1"], f1.bias) and _close(p["b2"], f2.bias)
    same_as_fuse(p)
    # the tap order is the convolution's: tap k = 3 ky + kx
    assert _close(p["taps"][5], fd.weight[:, 0, 1, 2])
    # the fold computes what the modules compute
    x = torch.randn(2, C, 5, 5)
    with torch.no_grad():
        want = ffn(dw(x))
        y1 = x + torch.nn.functional.conv2d(x, p["taps"].t().reshape(C, 1, 3, 3), p["dwb"], padding=1, groups=C)
        got = y1 + torch.einsum("oc,bchw->bohw", p["w2"].float(), torch.relu(
            torch.einsum("oc,bchw->bohw", p["w1"][:, :C].float(), y1) + p["b1"][None, :, None, None])) + p["b2"][None, :, None, None]
    assert _close(got, want, 2.0 ** -6)
    # new weights loaded after eval() are seen; so is an in-place edit
    sd = {k: v.clone() for k, v in ffn.state_dict().items()}
    sd["m.pw1.bn.running_var"] = sd["m.pw1.bn.running_var"] * 1.5
    ffn.load_state_dict(sd)
    p2 = evit_ffn.fold_dwffn(dw, ffn)
    assert p2 is not p and not torch.equal(p2["w1"], p["w1"]) and torch.equal(p2["w2"], p["w2"]) and torch.equal(p2["taps"], p["taps"])
    with torch.no_grad():
        dw.m.bn.bias.add_(1.0)
    p3 = evit_ffn.fold_dwffn(dw, ffn)
    assert p3 is not p2 and _close(p3["dwb"], p2["dwb"] + 1.0)
    fd, f1, f2 = dw.m.fuse(), ffn.m.pw1.fuse(), ffn.m.pw2.fuse()
    same_as_fuse(p3)
    # after replace_batchnorm the convolutions' own weight and bias are the operands
    ev.replace_batchnorm(dw)
    ev.replace_batchnorm(ffn)
    assert isinstance(dw.m, torch.nn.Conv2d) and isinstance(ffn.m.pw1, torch.nn.Conv2d)
    p4 = evit_ffn.fold_dwffn(dw, ffn)
    assert p4 is not p3
    for n in ("taps", "dwb", "w1", "b1", "w2", "b2"):
        assert _close(p4[n].float(), p3[n].float()), n
    with torch.no_grad():
        ffn.m.pw2.bias.mul_(2.0)
    assert _close(evit_ffn.fold_dwffn(dw, ffn)["b2"], 2.0 * p4["b2"])


def test_fold_pw_equals_fuse_and_pads_the_contraction():
    from cream_amd import efficientvit as ev, evit_ffn
    torch.manual_seed(1)
    conv = ev.Conv2d_BN(144, 96)
    with torch.no_grad():
        conv.bn.weight.normal_(1.0, 0.2)
        conv.bn.running_mean.normal_(0.0, 0.3)
        conv.bn.running_var.uniform_(0.5, 1.5)
    conv.eval()
    p, f = evit_ffn.fold_pw(conv), conv.fuse()
    assert (p["Cin"], p["Cout"]) == (144, 96) and tuple(p["w"].shape) == (96, 160) and not p["w"][:, 144:].any()
    assert _close(p["w"][:, :144].float(), f.weight[:, :, 0, 0], 2.0 ** -8) and _close(p["b"], f.bias)
    assert evit_ffn.fold_pw(conv) is p
    with torch.no_grad():
        conv.c.weight.mul_(0.5)
    assert _close(evit_ffn.fold_pw(conv)["w"].float(), 0.5 * p["w"].float(), 2.0 ** -8)
    assert evit_ffn.fold_pw(f)["w"].shape == p["w"].shape and _close(evit_ffn.fold_pw(f)["b"], p["b"])


def test_fused_blocks_switch_and_the_route_without_a_device():
    from test_efficientvit import build
    model = build()
    assert model.fused_blocks and not build(fused_blocks=False).fused_blocks
    x = torch.zeros(1, 3, 224, 224)
    assert not model.eval().is_tokens(x)                 # without a device nothing takes the token path
    model.fused_blocks = False
    assert not model.is_tokens(x)
