"""Host logic of the generalised fused iRPE attention (csrc/irpe_attn_x.hip; cream_irpe_attn2_* in include/cream_amd.h)
without a device: the entry points exist and refuse what is not implemented with an error code before anything is
launched, `irpe_fused.usable` decides as documented, and DETR's module keeps the composed path on the CPU."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import DETR_CASES, detr_fill, detr_inputs  # noqa: E402

BAD_ARG, TOO_LARGE = -1, -4


def _desc(head_dim=32, row_width=128, nb=81, L=140, k_table=True, q_table=False, v_table=False, backward=False):
    """A descriptor whose pointers are fake but non-null and 16-byte aligned: the argument check reads no memory."""
    from cream_amd import _lib
    x = _lib.IrpeAttn2Desc()
    d = x.base
    P = 0x10000
    d.q, d.k, d.v, d.out, d.lse = P, P, P, P, P
    d.sb, d.sn, d.sh = 8 * head_dim, 2 * 8 * head_dim, head_dim
    d.B, d.H, d.L, d.NP, d.nb = 2, 8, L, (L + 31) // 32 * 32, nb
    d.scale = head_dim ** -0.5
    if k_table:
        d.wk, d.idk, d.idk_t = P, P, P
    if q_table:
        d.wq, d.idq, d.idq_t = P, P, P
    if v_table:
        d.wv, d.idv, d.idv_t, d.sv = P, P, P, P
    if backward:
        d.dout, d.dq, d.dk, d.dv, d.delta, d.lkg, d.gg, d.dlk, d.dlq = (P,) * 9
        d.dsb, d.dsn, d.dsh = d.sb, d.sn, d.sh
    x.head_dim, x.row_width = head_dim, row_width
    return x


def test_new_entry_points_check_their_descriptor_without_a_device():
    from cream_amd import _lib
    lib = _lib.load()
    chk = lambda x, bwd=0: lib.cream_irpe_attn2_check(ctypes.byref(x), bwd)          # noqa: E731
    assert chk(_desc()) == 0 and chk(_desc(backward=True), 1) == 0                     # DETR's recipe
    assert chk(_desc(head_dim=64, nb=82, L=197)) == 0
    assert chk(_desc(row_width=64, nb=49, q_table=True, v_table=True)) == 0
    assert chk(_desc(), 1) == BAD_ARG                                                  # backward operands missing
    assert chk(_desc(head_dim=48)) == BAD_ARG
    assert chk(_desc(nb=129)) == BAD_ARG
    assert chk(_desc(row_width=64, nb=81)) == BAD_ARG                                  # nb > row width
    assert chk(_desc(row_width=96)) == BAD_ARG
    assert chk(_desc(q_table=True)) == BAD_ARG and chk(_desc(v_table=True)) == BAD_ARG  # 128 columns: k alone
    assert chk(_desc(k_table=False)) == BAD_ARG
    assert chk(_desc(L=2049)) == TOO_LARGE
    x = _desc()
    x.osb, x.osn = 256, 12                                                             # not a multiple of 8
    assert chk(x) == BAD_ARG
    x = _desc()
    x.base.dropout_p = 1.0
    assert chk(x) == BAD_ARG
    assert lib.cream_irpe_attn2_check(None, 0) == BAD_ARG
    # the launching calls return the same codes and launch nothing
    for bad in (_desc(head_dim=48), _desc(nb=129)):
        assert lib.cream_irpe_attn2_fwd(ctypes.byref(bad), None) == BAD_ARG
        assert lib.cream_irpe_attn2_bwd(ctypes.byref(bad), None) == BAD_ARG
    P = 0x10000
    tg = lambda xa, yc: lib.cream_irpe_table_grad2(P, P, 8, 8, 8, xa, P, 8, 8, 8, yc, 1, 1, 32, 1.0, None)   # noqa: E731
    assert tg(48, 64) == BAD_ARG and tg(32, 129) == BAD_ARG and tg(256, 32) == BAD_ARG
    assert lib.cream_irpe_table_grad2(None, P, 8, 8, 8, 32, P, 8, 8, 8, 128, 1, 1, 32, 1.0, None) == BAD_ARG


def test_desc_layout_matches_the_header():
    """The ctypes mirror embeds the existing descriptor unchanged and appends the new fields."""
    from cream_amd import _lib
    assert _lib.IrpeAttn2Desc.base.offset == 0 and _lib.IrpeAttn2Desc.base.size == ctypes.sizeof(_lib.IrpeAttnDesc)
    off = ctypes.sizeof(_lib.IrpeAttnDesc)
    assert off % 8 == 0
    assert (_lib.IrpeAttn2Desc.head_dim.offset, _lib.IrpeAttn2Desc.row_width.offset) == (off, off + 4)
    assert _lib.IrpeAttn2Desc.key_pad.offset == off + 8 and _lib.IrpeAttn2Desc.dosn.offset == off + 48
    assert ctypes.sizeof(_lib.IrpeAttn2Desc) == off + 56


def _mods(rpe_on, ratio, head_dim, method="product", mode="ctx"):
    from cream_amd import irpe as I
    return list(I.build_rpe(I.get_rpe_config(ratio=ratio, method=method, mode=mode, shared_head=True, skip=0, rpe_on=rpe_on),
                            head_dim=head_dim, num_heads=8))


def test_usable_decision_table(monkeypatch):
    from cream_amd import irpe as I, irpe_fused
    assert I.get_rpe_config(ratio=2.0, method='product', skip=0).rpe_k.num_buckets == 81
    cpu, dev = torch.device("cpu"), torch.device("cuda", 0)          # (a device object alone: nothing is initialised)
    k81, k49 = _mods("k", 2.0, 32), _mods("k", 1.9, 32)
    bf = torch.bfloat16
    assert not irpe_fused.usable(bf, cpu, 32, 140, k81) and not irpe_fused.usable(bf, cpu, 64, 197, [None] * 3)
    assert not irpe_fused.usable(torch.float32, dev, 32, 140, k81) and not irpe_fused.usable(torch.float16, dev, 32, 140, k49)
    for hd in (32, 64):
        assert irpe_fused.usable(bf, dev, hd, 140, _mods("k", 2.0, hd), key_padding=True, hw=(10, 14))
        assert irpe_fused.usable(bf, dev, hd, 140, _mods("k", 2.5, hd))                       # 121 buckets
        assert irpe_fused.usable(bf, dev, hd, 140, [None] * 3, key_padding=True)
        assert not irpe_fused.usable(bf, dev, hd, 140, _mods("k", 3.0, hd))                   # 169 buckets
        for on in ("q", "v", "qk", "kv", "qkv"):
            assert not irpe_fused.usable(bf, dev, hd, 140, _mods(on, 2.0, hd)), on            # above 64: k alone
            assert irpe_fused.usable(bf, dev, hd, 140, _mods(on, 1.9, hd), key_padding=True, hw=(10, 14)), on
        assert irpe_fused.usable(bf, dev, hd, 140, _mods("qk", 2.0, hd, mode="bias")) is False
        assert irpe_fused.usable(bf, dev, hd, 140, _mods("k", 2.0, hd, mode="bias"))
    for hd in (16, 48, 96, 128):
        assert not irpe_fused.usable(bf, dev, hd, 140, _mods("k", 1.9, hd)), hd
    assert not irpe_fused.usable(bf, dev, 32, 2049, [None] * 3) and irpe_fused.usable(bf, dev, 32, 2048, [None] * 3)
    assert not irpe_fused.usable(bf, dev, 32, 140, k81, dropout_p=1.0) and irpe_fused.usable(bf, dev, 32, 140, k81, dropout_p=0.1)
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")
    assert not irpe_fused.usable(bf, dev, 32, 140, k81)


def test_row_width_follows_the_bucket_count():
    from cream_amd import irpe_fused
    t = lambda nb: (None, 0, None, None, nb, False)          # noqa: E731
    assert irpe_fused.row_width((None, None, None)) == 64
    assert irpe_fused.row_width((None, t(49), t(49))) == 64 and irpe_fused.row_width((None, t(64), None)) == 64
    assert irpe_fused.row_width((None, t(65), None)) == 128 and irpe_fused.row_width((None, t(81), None)) == 128


def test_cpu_module_keeps_the_composed_path_whatever_need_weights_says():
    """On the CPU (and in fp32 anywhere) `need_weights=False` changes nothing but the second result."""
    from cream_amd.detr_attention import RPEMultiheadAttention
    from cream_amd.irpe import get_rpe_config
    tag = 'product_k_padmask'
    c = DETR_CASES[tag]
    att = RPEMultiheadAttention(256, 8, dropout=0.0, rpe_config=get_rpe_config(**c['kw']))
    detr_fill(att, seed=31)
    src, pos, gy, pad, _ = detr_inputs(tag, c)
    a, wa = att(src + pos, src + pos, src, key_padding_mask=pad, hw=c['hw'])
    b, wb = att(src + pos, src + pos, src, key_padding_mask=pad, need_weights=False, hw=c['hw'])
    assert torch.equal(a, b) and wa is not None and wb is None
    with torch.autocast("cpu", torch.bfloat16):
        d, _ = att(src + pos, src + pos, src, key_padding_mask=pad, need_weights=False, hw=c['hw'])
    assert torch.isfinite(d).all()
