"""The cascaded group attention kernel (cream_amd/csrc/cga_attn.hip) on the GPU, element by element against the fp64
reference of tests/cga_ref.py: with relu = 0 every head of every case is held to the reference of THAT head, fed the kernel's
own stored feat_{i-1} (the stored bf16 value is the cascaded value by design), within the bound derived from the rounding
points; relu = 1 is relu of that output bit for bit; two runs are bit-identical; bad descriptors return -1."""
import ctypes

import pytest
import torch

import cga_ref
from cga_ref import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_RUN = {}


def run(tag):
    """(x on the host, ops, pre-ReLU output, ReLU output, pre-ReLU output of a second run): computed once per case."""
    if tag not in _RUN:
        from cream_amd import cga_attn
        c = CASES[tag]
        x, ops = cga_ref.make_case(c, seed=sorted(CASES).index(tag))
        pack = cga_ref.to_pack(ops, DEV)
        if c["layout"] == "padded":                      # keep the slice a slice on the device
            xd = x._base.to(DEV)[:, :x.shape[1], :x.shape[2], :x.shape[3]] if x._base is not None else x.to(DEV)
        else:
            xd = x.to(DEV)
        assert xd.stride() == x.stride(), (xd.stride(), x.stride())
        assert xd.is_contiguous() == (c["layout"] != "padded")
        a = cga_attn.fwd_core(xd, pack, c["w"], ops["scale"], relu=False)
        r = cga_attn.fwd_core(xd, pack, c["w"], ops["scale"], relu=True)
        b = cga_attn.fwd_core(xd, pack, c["w"], ops["scale"], relu=False)
        torch.cuda.synchronize()
        _RUN[tag] = (x, ops, a.cpu(), r.cpu(), b.cpu())
    return _RUN[tag]


@pytest.mark.parametrize("tag", list(CASES))
def test_every_head_against_its_fp64_reference(tag):
    x, ops, out, _, _ = run(tag)
    assert out.shape == x.shape and out.dtype == torch.bfloat16 and bool(torch.isfinite(out.float()).all())
    res = cga_ref.check_heads(out, x, ops, CASES[tag]["w"])
    for i, ratio, err in res:
        print(f"[cga kernel {tag}] head {i}: worst error {err:.3e}, worst error / bound {ratio:.3f}")
    assert len(res) == CASES[tag]["h"] and all(ratio <= 1.0 for _, ratio, _ in res), res


@pytest.mark.parametrize("tag", list(CASES))
def test_relu_flag_and_determinism(tag):
    _, _, out, relu, again = run(tag)
    assert torch.equal(relu.view(torch.int16), torch.relu(out.float()).bfloat16().view(torch.int16))
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))
    assert bool((out.float() < 0).any())                 # the flag had something to do


def test_bad_descriptors_return_an_error_code():
    from cream_amd import _lib, cga_attn
    c = CASES["w7_h2_c48_2x2"]
    x, ops = cga_ref.make_case(c, seed=99)
    pack = cga_ref.to_pack(ops, DEV)
    xd = x.contiguous().to(DEV)
    out = torch.full(xd.shape, 7.0, dtype=torch.bfloat16, device=DEV)
    lib = _lib.load()

    def desc(**kw):
        d = _lib.CgaDesc()
        d.x, (d.xsb, d.xsy, d.xsx) = xd.data_ptr(), xd.stride()[:3]
        d.wqkv, d.bqkv, d.dw, d.dwb, d.ab = (pack[n].data_ptr() for n in ("wqkv", "bqkv", "dw", "dwb", "ab"))
        d.out = out.data_ptr()
        d.B, d.Hs, d.Ws, d.w, d.h, d.Cg, d.relu, d.scale = xd.shape[0], xd.shape[1], xd.shape[2], c["w"], c["h"], c["Cg"], 0, 0.25
        for i, k in enumerate(kw.pop("ks", c["ks"])):
            d.ks[i] = k
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(Cg=40), dict(Cg=128), dict(h=5), dict(w=9), dict(w=5), dict(Hs=13), dict(x=xd.data_ptr() + 2),
                dict(out=out.data_ptr() + 8), dict(wqkv=pack["wqkv"].data_ptr() + 4), dict(xsx=c["h"] * c["Cg"] + 2), dict(ks=(5, 2)),
                dict(ab=None)):
        assert lib.cream_cga_attn_fwd(ctypes.byref(desc(**bad)), st) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                      # nothing was launched
    assert lib.cream_cga_attn_fwd(ctypes.byref(desc()), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, cga_attn.fwd_core(xd, pack, c["w"], 0.25, relu=False))
