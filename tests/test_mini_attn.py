"""Fused Mini-DeiT attention with head transforms, the parts that need no GPU: the dispatch decision
(`mini_attn.usable_mixed`, from descriptors alone) and the argument checks of the C entry points."""
import ctypes

import pytest
import torch

CUDA = torch.device("cuda", 0)          # a descriptor: constructing it touches no device


def rpe_k(nb_ratio=1.9, mode='ctx', rpe_on='k', H=3):
    from cream_amd.irpe import build_rpe, get_rpe_config
    cfg = get_rpe_config(ratio=nb_ratio, method='product', mode=mode, shared_head=True, skip=0, rpe_on=rpe_on)
    return build_rpe(cfg, head_dim=64, num_heads=H)


def conv(H):
    return torch.zeros(H, H, 1, 1)


def decide(dtype=torch.bfloat16, device=CUDA, head_dim=64, H=3, L=196, rpes=None, dropout_p=0.0, wl=None, ww=None):
    from cream_amd import mini_attn
    rpes = rpe_k(H=H) if rpes is None else rpes
    return mini_attn.usable_mixed(dtype, device, head_dim, H, L, rpes, conv(H) if wl is None else wl,
                                  conv(H) if ww is None else ww, dropout_p=dropout_p)


@pytest.mark.parametrize("H,L", [(3, 196), (6, 196), (12, 196), (12, 576)])
def test_usable_for_the_published_configurations(H, L):
    rpes = rpe_k(H=H)
    assert rpes[0] is None and rpes[2] is None and rpes[1].num_buckets == 49
    assert decide(H=H, L=L, rpes=rpes)
    assert decide(H=H, L=L, rpes=(None, None, None))


def test_not_usable_outside_the_kernels_scope(monkeypatch):
    assert decide()
    assert not decide(device=torch.device("cpu"))
    assert not decide(dtype=torch.float32)
    assert not decide(H=13)
    assert not decide(head_dim=32)
    assert not decide(rpes=rpe_k(mode='bias'))
    r81 = rpe_k(nb_ratio=2.0)
    assert r81[1].num_buckets == 81
    assert not decide(rpes=r81)
    assert not decide(dropout_p=0.1)
    assert not decide(rpes=rpe_k(rpe_on='qk'))
    assert not decide(L=2049)
    assert not decide(wl=conv(3).bfloat16())
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")
    assert not decide()


def _desc(**kw):
    from cream_amd import _lib
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.MiniAttnDesc()
    d.q = d.k = d.v = d.out = d.lse = d.wl = d.ww = p
    d.sb, d.sn, d.sh = 8 * 3 * 3 * 64, 3 * 3 * 64, 64
    d.B, d.H, d.L, d.NP, d.nb, d.head_dim = 1, 3, 8, 32, 1, 64
    d.scale = 0.125
    for k, v in kw.items():
        setattr(d, k, v)
    return d, buf


@pytest.mark.parametrize("kw", [dict(H=13), dict(H=0), dict(head_dim=32), dict(nb=65), dict(wl=None), dict(ww=None),
                                dict(wl=None, ww=None), dict(NP=64), dict(q=None), dict(sn=3)])
def test_malformed_descriptors_are_refused_before_any_device_call(kw):
    """The checks come before the first HIP call, so the codes are the same on a machine without a GPU."""
    from cream_amd import _lib
    lib = _lib.load()
    d, _keep = _desc(**kw)
    assert lib.cream_mini_attn_fwd(ctypes.byref(d), None) == -1
    assert lib.cream_mini_attn_bwd(ctypes.byref(d), None) == -1


def test_too_long_and_missing_backward_buffers():
    from cream_amd import _lib
    lib = _lib.load()
    d, _keep = _desc(L=2049, NP=2080)
    assert lib.cream_mini_attn_fwd(ctypes.byref(d), None) == -4
    d, _keep = _desc()                                  # a valid forward descriptor without the backward's pointers
    assert lib.cream_mini_attn_bwd(ctypes.byref(d), None) == -1
    assert lib.cream_mini_attn_fwd(None, None) == -1


def test_misaligned_backward_outputs_are_refused():
    """dq / dk / dv rows are written as 8-byte vectors: an odd base pointer is an argument error, not a misaligned store."""
    from cream_amd import _lib
    lib = _lib.load()
    d, _keep = _desc()
    p = d.q
    d.dout = d.dq = d.dk = d.dv = d.delta = d.dwl_part = d.dww_part = p
    d.dsb, d.dsn, d.dsh = d.sb, d.sn, d.sh
    for name in ("dq", "dk", "dv"):
        setattr(d, name, p + 2)
        assert lib.cream_mini_attn_bwd(ctypes.byref(d), None) == -1, name
        setattr(d, name, p)
    d.delta = p + 2
    assert lib.cream_mini_attn_bwd(ctypes.byref(d), None) == -1
