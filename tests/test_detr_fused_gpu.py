"""DETR-with-iRPE's encoder self-attention on the fused iRPE kernels (csrc/irpe_attn_x.hip: 32-wide heads, up to 128
buckets on k, key padding mask) on the MI355X: which path runs, parity with the reference's own class (fixture
tests/golden/detr_rpe_attention.npz), an fp32 restatement sweep on the attention core, the exact semantics of the key
padding mask, dropout with the mask, determinism.  Measured worst values: profiles/NOTES_detr_fused.md."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from helpers import load_npz  # noqa: E402
from make_golden import DETR_CASES, detr_fill, detr_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def max_rel(a, b):
    """max |a - b| / max |b| (the measure of tests/helpers.py), on the device."""
    a, b = torch.as_tensor(a).detach().double().to(DEV), torch.as_tensor(b).detach().double().to(DEV)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _table(m):
    return m.lookup_table_bias if m.mode == "bias" else m.lookup_table_weight


def _params(mods):
    out = []
    for m in mods:
        if m is not None:
            out += [_table(p) for p in ((m.rp_rows, m.rp_cols) if hasattr(m, "rp_rows") else (m,))]
    return out


def _mods(rpe_on, mode, shared, method, ratio, skip, head_dim, H, seed=3):
    """[rpe_q, rpe_k, rpe_v] on the device with random tables that require a gradient."""
    from cream_amd import irpe as I
    if not rpe_on:
        return [None, None, None]
    kw = dict(ratio=ratio, method=method, shared_head=shared, skip=skip)
    cfg = I.get_rpe_config(mode=mode, rpe_on=rpe_on.replace("v", "") if mode == "bias" else rpe_on, **kw)
    if mode == "bias" and "v" in rpe_on:          # bias mode does not exist on the value side (irpe.py:468-470)
        cfg.rpe_v = I.get_rpe_config(mode="ctx", rpe_on="v", **kw).rpe_v
    mods = list(I.build_rpe(cfg, head_dim=head_dim, num_heads=H))
    g = torch.Generator().manual_seed(seed)
    for m in mods:
        if m is not None:
            m.to(DEV)
    for p in _params(mods):
        with torch.no_grad():
            p.copy_((0.3 * torch.randn(p.shape, generator=g)).to(DEV))
        p.requires_grad_()
    return mods


def _restatement(q, k, v, scale, mods, hw=None, pad=None, keep=None):
    """fp32 restatement of the attention core of rpe_attention_function.py:235-377 / rpe_vision_transformer.py:68-97 on
    the SAME bf16-rounded q, k, v (B, L, H, D): -> (out (B, L, H*D), lse (B, H, L)).  The lookups are rounded to bf16 as
    the reference's autocast matmul leaves them.  pad (B, L) bool: masked_fill(-inf) over the keys (:349-357)."""
    rnd = lambda t: t.to(torch.bfloat16).float()                               # noqa: E731
    q, k, v = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))              # (B, H, L, D)
    rq, rk, rv = mods
    L = q.shape[2]
    h_, w_ = hw if hw is not None else (None, None)
    qs = q * scale
    a = qs @ k.transpose(-2, -1)

    def ids_of(m):
        return m.bucket_ids_for(L, q.device, h_, w_).long()

    def w_of(m):
        w = m.lookup_table_weight.float()
        return w[0] if w.shape[0] == 1 else w.unsqueeze(0)

    def bias_of(m):
        return m.lookup_table_bias.float()[:, ids_of(m).flatten()].view(1, -1, L, L)

    def parts(m):
        return [] if m is None else ([m.rp_rows, m.rp_cols] if hasattr(m, "rp_rows") else [m])

    for m in parts(rk):
        if m.mode == "bias":
            a = a + bias_of(m)
        else:
            lk = rnd(qs @ w_of(m))
            a = a + lk.gather(-1, ids_of(m).expand(*lk.shape[:2], L, L))
    for m in parts(rq):
        if m.mode == "bias":
            a = a + bias_of(m).transpose(2, 3)
        else:
            lq = rnd((k * scale) @ w_of(m))
            a = a + lq.gather(-1, ids_of(m).expand(*lq.shape[:2], L, L)).transpose(2, 3)
    if pad is not None:
        a = a.masked_fill(pad[:, None, None, :], float("-inf"))
    p = a.softmax(-1)
    if keep is not None:
        p = p * keep
    out = p @ v
    for m in parts(rv):
        sv = torch.zeros(*p.shape[:3], m.num_buckets, device=p.device).scatter_add_(-1, ids_of(m).expand_as(p), p)
        out = out + sv @ w_of(m)
    return out.transpose(1, 2).reshape(q.shape[0], L, -1), torch.logsumexp(a, -1)


def _pad_mask(B, L, hw):
    """The right third of the last image's map (or, with a class token, the last third of its tokens) is padding."""
    m = torch.zeros(B, L, dtype=torch.bool)
    if hw is not None:
        h, w = hw
        g = torch.zeros(h, w, dtype=torch.bool)
        g[:, w - w // 3:] = True
        m[B - 1] = g.flatten()
    else:
        m[B - 1, L - L // 3:] = True
    return m.to(DEV)


# ---- 1. which path runs ----------------------------------------------------------------------------------------------

def _detr_module(tag, dropout=0.0):
    from cream_amd.detr_attention import RPEMultiheadAttention
    from cream_amd.irpe import get_rpe_config
    c = DETR_CASES[tag]
    att = RPEMultiheadAttention(256, 8, dropout=dropout, rpe_config=get_rpe_config(**c['kw']))
    detr_fill(att, seed=31)
    return att.to(DEV), c


def test_published_recipe_takes_the_fused_path():
    """--enc_rpe2d rpe-2.0-product-ctx-1-k (81 buckets on k, head_dim 32) with padded images, bf16 autocast,
    need_weights=False: the fused kernels run, the rpe_index operator (the composed path) does not."""
    from cream_amd import irpe as I, irpe_fused, timing
    from cream_amd.detr_attention import RPEMultiheadAttention
    att = RPEMultiheadAttention(256, 8, dropout=0.0, rpe_config=I.get_rpe_config(
        ratio=2.0, method='product', mode='ctx', shared_head=True, skip=0, rpe_on='k')).to(DEV)
    assert att.rpe_k.num_buckets == 81
    c = DETR_CASES['product_k_padmask']
    src, pos, gy, pad, _ = (t.to(DEV) if t is not None else None for t in detr_inputs('product_k_padmask', c))
    src.requires_grad_()
    pos.requires_grad_()
    timing.reset()
    timing.enable(True)
    with torch.autocast('cuda', torch.bfloat16):
        qk = src + pos
        out, wts = att(qk, qk, src, key_padding_mask=pad, need_weights=False, hw=c['hw'])
    (out.float() * gy).sum().backward()
    timing.enable(False)
    names = set(timing.summary())
    assert wts is None
    assert {"irpe_attn_fwd", "irpe_attn_bwd"} <= names and not {"rpe_index_fwd", "rpe_index_bwd"} & names, names
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in att.parameters())
    assert torch.isfinite(src.grad).all() and torch.isfinite(pos.grad).all()

    dev = torch.device(DEV)
    k81 = _mods("k", "ctx", True, "product", 2.0, 0, 32, 8)
    assert irpe_fused.usable(torch.bfloat16, dev, 32, 140, k81, key_padding=True, hw=(10, 14))
    assert irpe_fused.usable(torch.bfloat16, dev, 32, 140, k81)
    assert irpe_fused.usable(torch.bfloat16, dev, 64, 140, _mods("k", "ctx", True, "product", 2.0, 0, 64, 8))
    # not implemented: q / v above 64 buckets, more than 128 buckets, head_dim 48
    assert not irpe_fused.usable(torch.bfloat16, dev, 32, 140, _mods("qk", "ctx", True, "product", 2.0, 0, 32, 8))
    assert not irpe_fused.usable(torch.bfloat16, dev, 32, 140, _mods("kv", "ctx", True, "product", 2.0, 0, 32, 8))
    assert not irpe_fused.usable(torch.bfloat16, dev, 32, 140, _mods("q", "ctx", True, "product", 2.0, 0, 32, 8))
    k121 = _mods("k", "ctx", True, "product", 2.5, 0, 32, 8)
    assert k121[1].num_buckets == 121 and irpe_fused.usable(torch.bfloat16, dev, 32, 140, k121)
    assert not irpe_fused.usable(torch.bfloat16, dev, 32, 140, _mods("k", "ctx", True, "product", 3.0, 0, 32, 8))   # 169
    assert not irpe_fused.usable(torch.bfloat16, dev, 48, 140, _mods("k", "ctx", True, "product", 2.0, 0, 48, 8))
    assert not irpe_fused.usable(torch.float32, dev, 32, 140, k81)


def test_need_weights_attn_mask_and_fp32_stay_composed():
    from cream_amd import timing
    att, c = _detr_module('product_k_padmask')
    src, pos, gy, pad, _ = (t.to(DEV) if t is not None else None for t in detr_inputs('product_k_padmask', c))
    L = src.shape[0]
    for kw, cast in ((dict(need_weights=True), True), (dict(need_weights=False, attn_mask=torch.zeros(L, L, device=DEV)), True),
                     (dict(need_weights=False), False)):
        timing.reset()
        timing.enable(True)
        with torch.autocast('cuda', torch.bfloat16, enabled=cast):
            att(src + pos, src + pos, src, key_padding_mask=pad, hw=c['hw'], **kw)
        timing.enable(False)
        names = set(timing.summary())
        assert "rpe_index_fwd" in names and "irpe_attn_fwd" not in names, (kw, names)


# ---- 2. parity with the reference's class ------------------------------------------------------------------------------

def _run_module(att, c, tag, fused, fp32=False, drop_add=True):
    """One forward + backward of the module on the case's inputs -> dict of tensors (out, dsrc, dpos, every parameter
    gradient).  fused: bf16 autocast with need_weights=False (the fused kernels); else the composed path under the same
    autocast (need_weights=True keeps it composed), or — fp32 — the composed path without autocast."""
    from cream_amd import timing
    src, pos, gy, pad, add = (t.to(DEV) if t is not None else None for t in detr_inputs(tag, c))
    if drop_add:
        add = None
    src.requires_grad_()
    pos.requires_grad_()
    att.zero_grad(set_to_none=True)
    timing.reset()
    timing.enable(True)
    with torch.autocast('cuda', torch.bfloat16, enabled=not fp32):
        qk = src + pos
        out, _ = att(qk, qk, src, key_padding_mask=pad, attn_mask=add, need_weights=not fused, hw=c['hw'])
    (out.float() * gy).sum().backward()
    timing.enable(False)
    names = set(timing.summary())
    assert ("irpe_attn_fwd" in names) == fused and ("irpe_attn_bwd" in names) == fused, (fused, names)
    res = dict(out=out.detach().float(), dsrc=src.grad.clone(), dpos=pos.grad.clone())
    for n, p in att.named_parameters():
        res["grad|" + n] = p.grad.detach().float().clone()
    return res


def _sample(name, t):
    """The strided samples the fixture stores (tests/golden/make_golden.py `detr`)."""
    if name in ("out", "dsrc", "dpos"):
        return t[::6, :, ::2]
    n = name[len("grad|"):]
    return t if ("lookup" in n or t.dim() == 1) else t[::5, ::3]


@pytest.mark.parametrize("tag", list(DETR_CASES))
def test_fused_module_matches_reference_class(tag):
    """The module on the fused kernels (bf16 autocast) against the reference's own class in fp32: the fixture for
    `product_k_padmask` and `quant_bias_qk`; for `euc_qkv_addmask` (run here WITHOUT its additive mask, which the fused
    path does not take) a device fp32 run of the composed path.  The composed path under the SAME autocast is measured
    against the same reference in the same test.  Bounds: the attention core's own (tests/test_irpe_fused_gpu.py:
    1.3e-2 product, 5e-2 euclidean / quant); where the composed path under autocast itself exceeds that on a quantity
    (the bf16 projections around the core), the bound of that quantity is 2 x the composed path's error measured in
    this run (the rule of tests/test_irpe_fused_gpu.py:266-268).
    Measured on the MI355X (profiles/NOTES_detr_fused.md), worst quantity of each case, fused / composed under autocast:
    product_k_padmask 1.04e-2 (rpe_k table) / 1.25e-2 (dsrc, in_proj_weight) — bound 1.3e-2, nothing rescaled;
    euc_qkv_addmask 1.40e-2 (dsrc) / 1.59e-2 (in_proj_weight) — bound 5e-2; quant_bias_qk 4.37e-2 / 3.83e-2 (the two
    bias tables: 8 buckets, one of them holding most pairs — the near-cancelling sums the 5e-2 bound is for), every
    other quantity of that case <= 1.27e-2 / 1.39e-2 — bound 5e-2.  The composed path never exceeded a core bound, so
    the 2 x rule below did not apply in the recorded run."""
    att, c = _detr_module(tag)
    fused = _run_module(att, c, tag, fused=True)
    composed = _run_module(att, c, tag, fused=False)
    if tag == 'euc_qkv_addmask':
        ref = {k: _sample(k, v) for k, v in _run_module(att, c, tag, fused=False, fp32=True).items()}
    else:
        fix = {k[len(tag) + 1:]: v for k, v in load_npz("detr_rpe_attention.npz").items() if k.startswith(tag + "|")}
        assert list(att.state_dict().keys()) == json.loads(bytes(fix["keys"]).decode())
        ref = {k: torch.from_numpy(fix[k]) for k in fused}
    core = 1.3e-2 if c['kw']['method'] == 'product' else 5e-2
    bad = {}
    for k in fused:
        ef, ec = max_rel(_sample(k, fused[k]), ref[k]), max_rel(_sample(k, composed[k]), ref[k])
        bound = 2 * ec if ec > core else core
        print(f"[detr fused {tag}] {k:36s} fused {ef:.2e}  composed under autocast {ec:.2e}  bound {bound:.2e}")
        assert torch.isfinite(fused[k]).all(), k
        if not ef < bound:
            bad[k] = (ef, ec, bound)
    assert not bad, bad


# ---- 3. restatement sweep on the attention core --------------------------------------------------------------------

MAPS = {140: (10, 14), 196: (14, 14), 850: (25, 34)}
# (rpe_on, mode, shared, method, ratio, L, pad mask, head_dim): every value of every axis at least once with and without
# the mask.  product at ratio 1.9 / skip 0: 49 buckets, ratio 2.0: 81 (k only: above 64 buckets q and v are not built)
SWEEP = [
    ("", "ctx", True, "product", 1.9, 140, False, 32), ("", "ctx", True, "product", 1.9, 196, True, 32),
    ("k", "ctx", True, "product", 2.0, 140, True, 32), ("k", "ctx", True, "product", 2.0, 850, False, 32),
    ("k", "ctx", False, "product", 2.0, 196, False, 32), ("k", "bias", True, "product", 2.0, 850, True, 32),
    ("k", "bias", False, "product", 2.0, 140, False, 32), ("k", "ctx", False, "product", 2.0, 196, True, 32),
    ("k", "ctx", True, "product", 2.5, 140, True, 32),                                    # 121 buckets
    ("qk", "ctx", False, "product", 1.9, 196, True, 32), ("qk", "bias", True, "product", 1.9, 140, False, 32),
    ("qk", "ctx", True, "euc", 1.9, 850, False, 32),
    ("qkv", "ctx", True, "product", 1.9, 850, True, 32), ("qkv", "ctx", False, "product", 1.9, 140, False, 32),
    ("qkv", "bias", False, "euc", 1.9, 196, True, 32), ("qkv", "ctx", True, "euc", 1.9, 140, False, 32),
    ("qkv", "ctx", True, "cross", 1.9, 196, False, 32), ("k", "ctx", False, "cross", 1.9, 140, True, 32),
    ("qk", "bias", False, "cross", 1.9, 850, True, 32), ("v", "ctx", True, "product", 1.9, 140, True, 32),
    ("q", "ctx", False, "product", 1.9, 196, False, 32), ("kv", "ctx", True, "product", 1.9, 140, False, 32),
    # head_dim 64 with 81 buckets on k (skip = 1: 82): the ratio-2.0 DeiT configurations
    ("k", "ctx", True, "product", 2.0, 197, False, 64), ("k", "ctx", False, "product", 2.0, 577, True, 64),
    ("k", "bias", True, "product", 2.0, 197, True, 64),
    # head_dim 64 at <= 64 buckets WITH the mask (without one these shapes run csrc/irpe_attn.hip)
    ("qkv", "ctx", True, "product", 1.9, 197, True, 64),
]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "-".join(str(x) for x in c))
def test_fused_core_matches_restatement(case):
    from cream_amd import irpe_fused
    rpe_on, mode, shared, method, ratio, L, masked, D = case
    B, H = 2, 3
    hw = MAPS.get(L)
    torch.manual_seed(11)
    mods = _mods(rpe_on, mode, shared, method, ratio, 0 if hw else 1, D, H)
    pad = _pad_mask(B, L, hw) if masked else None
    assert irpe_fused.usable(torch.bfloat16, torch.device(DEV), D, L, mods, key_padding=masked, hw=hw)
    qkv = (0.8 * torch.randn(B, L, 3, H, D, device=DEV)).to(torch.bfloat16).requires_grad_()
    gy = torch.randn(B, L, H * D, device=DEV).to(torch.bfloat16)
    scale = D ** -0.5
    q, k, v = qkv.unbind(2)
    if masked or hw is not None:
        y = irpe_fused.attention_qkv(q, k, v, scale, *mods, key_padding_mask=pad, hw=hw)
    else:                                           # the packed entry: routed to the wide kernels by head_dim / bucket count
        y = irpe_fused.attention(qkv, scale, *mods)
    params = _params(mods)
    got = torch.autograd.grad(y, [qkv] + params, gy)
    ref, _ = _restatement(q, k, v, scale, mods, hw, pad)
    want = torch.autograd.grad(ref, [qkv] + params, gy.float())
    errs = dict(y=max_rel(y.float(), ref))
    for name, a, b in zip(["dq", "dk", "dv"], got[0].float().unbind(2), want[0].float().unbind(2)):
        errs[name] = max_rel(a, b)
    for i, (a, b) in enumerate(zip(got[1:], want[1:])):
        assert a.shape == b.shape
        errs[f"dW{i}"] = max_rel(a.float(), b.float())
    print(f"[detr fused core {'-'.join(str(x) for x in case)}]", {k_: f"{v_:.2e}" for k_, v_ in errs.items()})
    assert all(torch.isfinite(t).all() for t in got)
    if masked:                                      # padded keys: no gradient at all
        assert float(got[0][:, :, 1:][pad].abs().max()) == 0.0
    # the bounds of tests/test_irpe_fused_gpu.py for the same arithmetic at 64 wide: product 1.3e-2; euclidean / quant / cross
    # (few buckets, near-cancelling bucket gradients) 5e-2
    bound = 1.3e-2 if method == "product" else 5e-2
    for k_, v_ in errs.items():
        assert v_ < bound, (k_, v_, errs)


# ---- 4. the mask, exactly ----------------------------------------------------------------------------------------------

def _core_inputs(tag='product_k_padmask', H=8, D=32, rpe_on="k", ratio=2.0, seed=5):
    c = DETR_CASES[tag]
    L = c['hw'][0] * c['hw'][1]
    pad = detr_inputs(tag, c)[3].to(DEV)
    torch.manual_seed(seed)
    mods = _mods(rpe_on, "ctx", True, "product", ratio, 0, D, H)
    q, k, v = ((0.8 * torch.randn(2, L, H, D, device=DEV)).to(torch.bfloat16) for _ in range(3))
    gy = torch.randn(2, L, H * D, device=DEV).to(torch.bfloat16)
    return c['hw'], L, pad, mods, q, k, v, gy


def _core_run(q, k, v, gy, mods, hw, pad, drop_p=0.0, seed=0):
    """fwd_core_x + bwd_core_x -> dict of every result, the per-image table-gradient partials included."""
    from cream_amd import irpe_fused
    L = q.shape[1]
    terms = tuple(irpe_fused._term(r, L, q.device, hw) for r in mods)
    kp = irpe_fused._pad_bytes(pad, q.shape[0], L)
    scale = q.shape[3] ** -0.5
    out, lse, sv = irpe_fused.fwd_core_x(q, k, v, scale, terms, kp, drop_p, seed)
    parts = {}
    (dq, dk, dv), res = irpe_fused.bwd_core_x(gy, q, k, v, out, lse, sv, scale, terms, kp, drop_p, seed, partials=parts)
    r = dict(out=out, lse=lse, dq=dq.clone(), dk=dk.clone(), dv=dv.clone())
    r.update({"dW" + n: t for n, t in zip("qkv", res) if t is not None})
    r.update({"part_" + n: t for n, t in parts.items()})
    return r


@pytest.mark.parametrize("rpe_on,ratio", [("k", 2.0), ("qkv", 1.9)])
def test_key_padding_mask_is_exact(rpe_on, ratio):
    hw, L, pad, mods, q, k, v, gy = _core_inputs(rpe_on=rpe_on, ratio=ratio)
    assert pad[1].any() and not pad[0].any()
    a = _core_run(q, k, v, gy, mods, hw, pad)
    assert all(torch.isfinite(t).all() for t in a.values())
    # (a) padded keys receive exactly nothing
    assert float(a["dk"][pad].abs().max()) == 0.0 and float(a["dv"][pad].abs().max()) == 0.0
    # (b) what the padded keys hold does not matter: other finite values there leave every result at the real positions
    # (and every table gradient) bit-identical
    k2, v2 = k.clone(), v.clone()
    k2[pad] = (k2[pad].float() * 1000).to(torch.bfloat16)
    v2[pad] = (v2[pad].float() * -1000).to(torch.bfloat16)
    b = _core_run(q, k2, v2, gy, mods, hw, pad)
    real = ~pad
    for n in a:
        if n in ("dq", "dk", "dv"):
            assert torch.equal(a[n][real], b[n][real]), n
        else:
            assert torch.equal(a[n], b[n]), n
    assert float(b["dk"][pad].abs().max()) == 0.0 and float(b["dv"][pad].abs().max()) == 0.0
    # (c) image 0 of the batch = image 0 alone, bit for bit (table gradients: the per-image partials)
    s = _core_run(q[:1], k[:1], v[:1], gy[:1], mods, hw, pad[:1])
    for n in a:
        if n.startswith("dW"):
            continue
        assert torch.equal(a[n][:1], s[n]), n
    # the mask does something: without it image 1 differs, image 0 does not
    u = _core_run(q, k, v, gy, mods, hw, None)
    assert torch.equal(u["out"][:1], a["out"][:1]) and not torch.equal(u["out"][1:], a["out"][1:])


@pytest.mark.parametrize("rpe_on,ratio", [("k", 2.0), ("qkv", 1.9)])
def test_key_padding_mask_with_dropout_matches_masked_restatement(rpe_on, ratio):
    """(d) dropout 0.1 with the pad mask against the masked restatement with the kernels' keep mask
    (irpe_fused.dropout_keep_mask); bound 1.5e-2 as tests/test_irpe_fused_gpu.py's dropout test."""
    import numpy as np
    from cream_amd import irpe_fused
    hw, L, pad, mods, q, k, v, gy = _core_inputs(rpe_on=rpe_on, ratio=ratio)
    rate, seed = 0.1, 4321
    keep_np = irpe_fused.dropout_keep_mask(seed, 2, 8, L) >= np.uint32(irpe_fused.dropout_threshold(rate))
    keep = torch.from_numpy(keep_np).to(DEV).float() / (1.0 - float(np.float32(rate)))
    qkv = [t.clone().requires_grad_() for t in (q, k, v)]
    y = irpe_fused.attention_qkv(*qkv, 32 ** -0.5, *mods, key_padding_mask=pad, dropout_p=rate, seed=seed, hw=hw)
    params = _params(mods)
    got = torch.autograd.grad(y, qkv + params, gy)
    ref, _ = _restatement(*qkv, 32 ** -0.5, mods, hw, pad, keep=keep)
    want = torch.autograd.grad(ref, qkv + params, gy.float())
    names = ["dq", "dk", "dv"] + [f"dW{i}" for i in range(len(params))]
    errs = dict(y=max_rel(y.float(), ref), **{n: max_rel(a.float(), b.float()) for n, a, b in zip(names, got, want)})
    print(f"[detr fused dropout + mask, rpe on {rpe_on}]", {k_: f"{v_:.2e}" for k_, v_ in errs.items()})
    assert float(got[1][pad].abs().max()) == 0.0 and float(got[2][pad].abs().max()) == 0.0
    for k_, v_ in errs.items():
        assert v_ < 1.5e-2, (k_, v_, errs)
    assert max_rel(y.float(), _restatement(q, k, v, 32 ** -0.5, mods, hw, pad)[0].detach()) > 5e-2     # a statement about the mask


def test_lse_and_out_match_masked_softmax():
    """lse of the kernels = logsumexp over the real keys only."""
    hw, L, pad, mods, q, k, v, gy = _core_inputs()
    a = _core_run(q, k, v, gy, mods, hw, pad)
    ref, lse = _restatement(q, k, v, 32 ** -0.5, mods, hw, pad)
    assert max_rel(a["lse"], lse) < 1e-3 and max_rel(a["out"].float(), ref) < 1.3e-2


# ---- 5. determinism ---------------------------------------------------------------------------------------------------

def test_two_runs_are_bit_identical():
    hw, L, pad, mods, q, k, v, gy = _core_inputs(rpe_on="qkv", ratio=1.9)
    a = _core_run(q, k, v, gy, mods, hw, pad, drop_p=0.1, seed=99)
    b = _core_run(q, k, v, gy, mods, hw, pad, drop_p=0.1, seed=99)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    att, c = _detr_module('product_k_padmask', dropout=0.1)
    att.train()
    res = []
    for _ in range(2):
        torch.manual_seed(7)
        res.append(_run_module(att, c, 'product_k_padmask', fused=True))
    for n in res[0]:
        assert torch.equal(res[0][n], res[1][n]), n
