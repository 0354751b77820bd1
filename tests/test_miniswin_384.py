"""Mini-Swin at 384 (window 12) without a GPU: what `usable_mix_large_window` accepts, the library's argument check and partial
size, the routing of `miniswin.WindowAttention.route` from descriptors alone, and the 384 recipe's shapes."""
import ctypes

import pytest
import torch

RECIPE = [(12, 96, 96, 4), (12, 48, 48, 8), (12, 24, 24, 16), (12, 12, 12, 32)]      # (w, Hs, Ws, H) of the four stages


def _mods(H, bias=True):
    return torch.nn.Linear(H, H, bias=bias), torch.nn.Linear(H, H, bias=bias)


def _table(w, H):
    return torch.zeros((2 * w - 1) ** 2, H)


def _usable(w=12, H=4, dtype=torch.bfloat16, device="cuda", head_dim=32, table=None, mods=None, **kw):
    from cream_amd import window_attn_mix_large as W
    table = _table(w, H) if table is None else table
    pl, pw = mods if mods is not None else _mods(max(H, 1))
    return W.usable_mix_large_window(dtype, device, head_dim, H, w, table, pl, pw, **kw)


def test_usable_truth_table(monkeypatch):
    monkeypatch.delenv("CREAM_IRPE_FUSED", raising=False)
    from cream_amd import window_attn_mix_large as W
    assert (W.MIN_WINDOW, W.MAX_WINDOW, W.MAX_HEADS) == (9, 12, 16)
    for w, Hs, Ws, H in RECIPE:
        assert _usable(w=w, H=H) == (H <= 16), (w, H)          # 32 heads (stage 4) are refused
    assert all(_usable(w=w, H=3) for w in (9, 10, 11, 12))
    assert not _usable(w=8, H=3) and not _usable(w=13, H=3)
    assert _usable(H=1) and _usable(H=16)
    assert not _usable(H=0) and not _usable(H=17) and not _usable(H=33)
    assert not _usable(dtype=torch.float32) and not _usable(dtype=torch.float16)
    assert not _usable(device="cpu")
    assert not _usable(dropout_p=0.1) and _usable(dropout_p=0.0)
    assert not _usable(head_dim=64)
    assert not _usable(mods=_mods(4, bias=False))                                       # missing bias
    assert not _usable(mods=(None, None)) and not _usable(mods=(_mods(4)[0], None))       # no head transforms: another family
    assert not _usable(mods=_mods(5))                                                   # transforms of another head count
    assert not _usable(table=torch.zeros(4, 23 * 23).t())                               # non-contiguous table
    assert not _usable(table=_table(12, 4).double()) and not _usable(table=_table(11, 4))
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")                                         # the switch
    assert not _usable()
    monkeypatch.setenv("CREAM_IRPE_FUSED", "1")
    assert _usable()


def _desc(H=4, w=12, Hs=24, Ws=24, B=1, shift=6, ms=6, head_dim=32, mix=True):
    from cream_amd import _lib
    d = _lib.WindowAttnMixLargeDesc()
    for n in ("q", "k", "v", "out", "lse", "table", "dout", "dq", "dk", "dv", "delta", "part"):
        setattr(d, n, 0x10000)                                # any aligned non-null pointer: only checked, never read
    if mix:
        d.wl = d.bl = d.ww = d.bw = 0x10000
    d.sb, d.sn, d.sh = Hs * Ws * 3 * H * 32, 3 * H * 32, 32
    d.dsb, d.dsn, d.dsh = d.sb, d.sn, d.sh
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = B, H, Hs, Ws, w, shift, ms, head_dim
    d.scale, d.part_blocks = 0.25, 1
    return d


def test_check_and_part_size_return_codes_without_a_device():
    from cream_amd import _lib
    lib = _lib.load()
    BAD = -1

    def check(bwd=0, **kw):
        return lib.cream_window_attn_mix_large_check(ctypes.byref(_desc(**kw)), bwd)
    assert check() == 0 and check(bwd=1) == 0
    assert all(check(w=w, Hs=2 * w, Ws=2 * w, shift=w // 2, ms=w // 2) == 0 for w in (9, 10, 11, 12))
    assert all(check(H=H) == 0 for H in (1, 16))
    for kw in (dict(w=8, Hs=16, Ws=16, shift=4, ms=4), dict(w=13, Hs=26, Ws=26), dict(H=0), dict(H=17), dict(H=32), dict(H=33),
               dict(head_dim=64), dict(mix=False), dict(Hs=25), dict(shift=12), dict(ms=12), dict(shift=-1), dict(B=-1)):
        assert check(**kw) == BAD and check(bwd=1, **kw) == BAD, kw
    assert lib.cream_window_attn_mix_large_check(None, 0) == BAD
    d = _desc()
    d.part_blocks = 0
    assert lib.cream_window_attn_mix_large_check(ctypes.byref(d), 1) == BAD and lib.cream_window_attn_mix_large_check(ctypes.byref(d), 0) == 0
    d = _desc()
    d.wl = None                                               # three of the four transforms
    assert lib.cream_window_attn_mix_large_check(ctypes.byref(d), 0) == BAD
    # refused before any HIP call: no device is needed for these either
    assert lib.cream_window_attn_mix_large_fwd(ctypes.byref(_desc(H=32)), None) == BAD
    assert lib.cream_window_attn_mix_large_bwd(ctypes.byref(_desc(w=13, Hs=26, Ws=26)), None) == BAD
    assert lib.cream_window_attn_mix_large_blocks(ctypes.byref(_desc(H=17))) == BAD
    assert lib.cream_window_attn_mix_large_fwd(ctypes.byref(_desc(B=0)), None) == 0       # B == 0: a no-op
    assert lib.cream_window_attn_mix_large_bwd(ctypes.byref(_desc(B=0)), None) == 0
    for H, w in ((1, 9), (3, 12), (16, 12), (8, 10)):
        n = (2 * w - 1) ** 2 * H + 2 * H * H + 2 * H
        assert lib.cream_window_attn_mix_large_part_size(H, w) == n
    assert lib.cream_window_attn_part_size(16, 8, 1) == 15 * 15 * 16 + 2 * 256 + 32       # the layout it follows
    for H, w in ((0, 12), (17, 12), (32, 12), (4, 8), (4, 13)):
        assert lib.cream_window_attn_mix_large_part_size(H, w) == BAD, (H, w)


class _FakeQkv:
    """What `route` reads of the projection: its dtype and device (no tensor on a device is made)."""

    def __init__(self, dtype=torch.bfloat16, device="cuda:0"):
        self.dtype, self.device = dtype, torch.device(device)


def _attn(H, w, mix):
    from cream_amd import miniswin
    a = miniswin.WindowAttention(H * 32, (w, w), H)
    pl, pw = _mods(H) if mix else (None, None)
    return a, pl, pw


def test_routing_from_descriptors_alone(monkeypatch):
    monkeypatch.delenv("CREAM_IRPE_FUSED", raising=False)
    from cream_amd import window_attn_mix_large as W
    # the default sets hold measured recipe shapes only
    assert W.ACCEPTED <= set(RECIPE) and W.PLAIN_ACCEPTED <= set(RECIPE)
    assert not any(s[3] > W.MAX_HEADS for s in W.ACCEPTED)
    monkeypatch.setattr(W, "ACCEPTED", frozenset({(12, 24, 24, 16)}))
    monkeypatch.setattr(W, "EXCLUDED", frozenset())
    monkeypatch.setattr(W, "PLAIN_ACCEPTED", frozenset({(12, 24, 24, 16)}))
    monkeypatch.setattr(W, "PLAIN_EXCLUDED", frozenset())
    q = _FakeQkv()
    a, pl, pw = _attn(16, 12, True)
    assert a.route(q, 12, 24, 24, pl, pw) == "mix_large"                         # a recipe shape routes
    assert a.route(q, 12, 24, 36, pl, pw) is None                                # the same block on an unmeasured map
    assert a.route(_FakeQkv(torch.float32), 12, 24, 24, pl, pw) is None
    assert a.route(_FakeQkv(device="cpu"), 12, 24, 24, pl, pw) is None
    assert a.route(q, 12, 24, 24, None, None) == "large"                         # the plain teacher's block
    a2, pl2, pw2 = _attn(2, 12, True)
    assert a2.route(q, 12, 12, 24, pl2, pw2) is None                             # (12, 12, 24, 2) stays composed
    W.ACCEPTED |= {(12, 12, 24, 2)}                                              # ... until a caller adds it
    assert a2.route(q, 12, 12, 24, pl2, pw2) == "mix_large"
    monkeypatch.setattr(W, "EXCLUDED", frozenset({(12, 12, 24, 2)}))
    assert a2.route(q, 12, 12, 24, pl2, pw2) is None
    assert a2.route(q, 12, 12, 24, None, None) is None
    W.PLAIN_ACCEPTED |= {(12, 12, 24, 2)}
    assert a2.route(q, 12, 12, 24, None, None) == "large"
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")
    assert a.route(q, 12, 24, 24, pl, pw) is None and a.route(q, 12, 24, 24, None, None) is None
    monkeypatch.delenv("CREAM_IRPE_FUSED")
    a32, pl32, pw32 = _attn(32, 12, True)
    W.ACCEPTED |= {(12, 12, 12, 32)}
    assert a32.route(q, 12, 12, 12, pl32, pw32) is None                          # 32 mixed heads are not covered, listed or not
    a7, pl7, pw7 = _attn(3, 7, True)
    assert a7.route(q, 7, 14, 14, pl7, pw7) == "window"                          # window 7 keeps its kernels


def test_the_384_recipe_builds_with_its_shapes():
    from cream_amd import miniswin
    m = miniswin.mini_swin('base', img_size=384, window_size=12, num_classes=10)
    got = []
    for layer in m.layers:
        for blk in layer.blocks:
            assert blk.is_transform_heads and blk.share_num == 2
            got.append((blk.window_size,) + tuple(blk.input_resolution) + (blk.num_heads,))
            assert blk.attn.relative_position_bias_table.shape == (23 * 23, blk.num_heads)
    assert sorted(set(got), reverse=True) == sorted(RECIPE, reverse=True), got
    assert [b.shift_size for layer in m.layers for b in layer.blocks[:1]] == [6, 6, 6, 0]     # the last stage is one window
