"""The depthwise 3 x 3 + FFN kernel and the proj + residual kernel (cream_amd/csrc/evit_ffn.hip) on the GPU, element by
element against the fp64 reference of tests/evit_ffn_ref.py: every element of every case within the bound derived from the
rounding points; two runs bit-identical; the three layouts of x give equal bits for equal values; bad descriptors launch
nothing."""
import ctypes

import pytest
import torch

import evit_ffn_ref as R
from evit_ffn_ref import CASES, LAYOUTS, PW_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_RUN = {}


def run(tag):
    """(x on the host, ops, reference, bound, {layout: output}, output of a second run in the case's layout): once per case."""
    if tag not in _RUN:
        from cream_amd import evit_ffn
        c = CASES[tag]
        seed = sorted(CASES).index(tag)
        x, ops = R.make_case(c, seed=seed)
        pack = R.to_pack(ops, DEV)
        outs = {}
        for layout in LAYOUTS:
            xl = R.make_case(c, seed=seed, layout=layout)[0]
            outs[layout] = evit_ffn.fwd_dwffn(R.to_device(xl, DEV, layout), pack)
        again = evit_ffn.fwd_dwffn(R.to_device(x, DEV, c["layout"]), pack)
        torch.cuda.synchronize()
        _RUN[tag] = (x, ops, R.reference(x, ops), R.bound(x, ops), {k: v.cpu() for k, v in outs.items()}, again.cpu())
    return _RUN[tag]


@pytest.mark.parametrize("tag", list(CASES))
def test_every_element_against_the_fp64_reference(tag):
    x, ops, ref, bnd, outs, _ = run(tag)
    out = outs[CASES[tag]["layout"]]
    assert out.shape == x.shape and out.dtype == torch.bfloat16 and out.is_contiguous() and bool(torch.isfinite(out.float()).all())
    ratio, err = R.worst(out, ref, bnd)
    print(f"[evit dwffn kernel {tag}] worst error {err:.3e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("tag", list(CASES))
def test_reruns_and_layouts_are_bit_identical(tag):
    _, _, _, _, outs, again = run(tag)
    first = outs[CASES[tag]["layout"]].view(torch.int16)
    assert torch.equal(first, again.view(torch.int16))
    for layout in LAYOUTS:
        assert torch.equal(first, outs[layout].view(torch.int16)), layout


@pytest.mark.parametrize("tag", list(PW_CASES))
def test_pw_residual_against_the_fp64_reference(tag):
    from cream_amd import evit_ffn
    c = PW_CASES[tag]
    a, res, ops = R.make_pw_case(c, seed=sorted(PW_CASES).index(tag))
    pack = R.to_pw_pack(ops, DEV)
    ad, rd = R.to_device(a, DEV, c["la"]), R.to_device(res, DEV, c["lr"])
    out, again = evit_ffn.fwd_pw_residual(ad, rd, pack), evit_ffn.fwd_pw_residual(ad, rd, pack)
    plain = evit_ffn.fwd_pw_residual(ad.contiguous(), rd.contiguous(), pack)
    assert out.shape == res.shape and out.dtype == torch.bfloat16 and out.is_contiguous()
    ratio, err = R.worst(out, R.pw_reference(a, res, ops), R.pw_bound(a, res, ops))
    print(f"[evit pw kernel {tag}] worst error {err:.3e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)) and torch.equal(out.view(torch.int16), plain.view(torch.int16))


def test_bad_descriptors_launch_nothing_and_uncovered_shapes_raise():
    from cream_amd import _lib, evit_ffn
    c = CASES["g_c32_3x5"]
    x, ops = R.make_case(c, seed=99)
    pack = R.to_pack(ops, DEV)
    xd = x.to(DEV)
    out = torch.full(xd.shape, 7.0, dtype=torch.bfloat16, device=DEV)
    lib = _lib.load()

    def desc(**kw):
        d = _lib.EvitDwffnDesc()
        d.x, (d.xsb, d.xsy, d.xsx, d.xsc) = xd.data_ptr(), xd.stride()
        d.taps, d.dwb, d.w1, d.b1, d.w2, d.b2 = (pack[n].data_ptr() for n in ("taps", "dwb", "w1", "b1", "w2", "b2"))
        d.out = out.data_ptr()
        d.B, d.H, d.W, d.C, d.Ch = c["B"], c["H"], c["W"], c["C"], c["Ch"]
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    st = torch.cuda.current_stream().cuda_stream
    for code, bad in ((-7, dict(C=24)), (-7, dict(Ch=48)), (-7, dict(H=0)), (-1, dict(x=xd.data_ptr() + 2)), (-1, dict(out=None)),
                      (-1, dict(w1=pack["w1"].data_ptr() + 4)), (-5, dict(xsc=2)), (-6, dict(xsx=c["C"] + 2)), (-6, dict(xsx=16))):
        assert lib.cream_evit_dwffn_fwd(ctypes.byref(desc(**bad)), st) == code, bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                      # nothing was launched
    assert lib.cream_evit_dwffn_fwd(ctypes.byref(desc()), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, evit_ffn.fwd_dwffn(xd, pack))
    with pytest.raises(RuntimeError):                    # no fall-back in the module: a view the kernel does not take raises
        evit_ffn.fwd_dwffn(xd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), pack)
    with pytest.raises(RuntimeError):
        evit_ffn.fwd_pw_residual(torch.zeros(1, 2, 2, 24, dtype=torch.bfloat16, device=DEV),
                                 torch.zeros(1, 2, 2, 32, dtype=torch.bfloat16, device=DEV),
                                 dict(Cin=24, Cout=32, w=pack["w1"], b=pack["b1"]))
