"""fp64 reference, rounding model, per-element bounds and the shared case list for the kernel-level tests of
csrc/window_attn_xl.hip (fused window attention for windows of 15x15 .. 32x32: keys and values stream through LDS).

`xl_reference` is the operation written out per window in fp64 from its definition — S = (s q) k^T + T[rel], P = softmax S,
O = P v, delta = sum_j P dP, dS = P (dP - delta), dq = s dS k, dk = dS^T (s q), dv = P^T dO, dT[u] = sum_{rel = u} dS — with
the window partition of attn_mix_ref and Swin's `relative_position_index`; nothing in it follows the kernels' index arithmetic
(no tiles, no chunks, no padding).  tests/test_window_xl_ref_cpu.py holds it against the fp64 AUTOGRAD statement of
attn_mix_ref.window_reference.  It also carries the injected faults (XL_FAULTS).

`xl_model` is the same arithmetic with a bf16 rounding at exactly the places where the kernels have one; `xl_ref_and_bound` is
the reference together with a bound per output element, computed once per case and shared.

The kernels keep the arithmetic of window_attn_large.hip — the same two-pass softmax (pass 1: a running (max, sum) per lane over
the key tiles; pass 2: P = exp(S - lse)), the same rounding points L1 .. L4 of tests/window_large_ref.py, the same fused
multiply-add chains for delta — and only change where a key tile comes from (a streamed chunk instead of the resident copy),
which rounds nothing.  So the bound is the derivation of window_large_ref.py, step by step, with NT up to 32 and NP up to 1024
in its counts, and ONE constant restated: `__logf` now sees l in [1, 1024], and 3 ulps of log 1024 = 6.93 are 24 u (u = 2^-24;
the ulp of [4, 8) is 8 u) where log 224 needed 17 u:
    E(lse) = sum_j P e_S + u (|lse| + NP / 2 + 5 NT + 34)
A term of l passes through at most 16 + NT + 1 additions, NT + 1 multiplications by an exp2f of 2 ulps, its own exp2f and the
rounding of its argument: 3 NT + 23 roundings, under NP / 2 + 5 NT + 10 for every NT.  d table: a thread's chain per (query block,
key tile), then onto the workgroup's entry, then the caller's sum of the partials — every term passes through at most `pairs`
additions, as before.  First-order throughout.  No constant is fitted.
"""
from collections import namedtuple
from functools import lru_cache

import torch

from attn_mix_ref import (SEED, TINY, U32, from_windows, hu, ident, bf16, relative_position_index, scaled_bf16, to_windows,
                          worst_ratio)  # noqa: F401  (worst_ratio: for the tests)
from window_large_ref import _core, _dtable

_XCase = namedtuple("XCase", "group B H Hs Ws w scale")


class XCase(_XCase):
    """The fields of window_large_ref.LCase that exist here; the others are constants (for attn_mix_ref.window_reference)."""
    __slots__ = ()
    shift = 0
    ms = 0
    mixed = False


XL_FAULTS = ("rel_off_by_one_row", "padding_counted", "delta_misses_a_tile", "dT_wrong_diagonal", "scale_twice")
S0 = 32 ** -0.5


def _xl_cases():
    cs = []
    # 225 tokens: 31 padded keys in the last tile; 256: exact tiles; 289: one real key in the last tile; 576; 961 and 1024: the
    # longest stream (16 chunks) and the largest table column (3969)
    for w in (15, 16, 17, 24, 31, 32):
        cs.append(XCase("size", 1, 3, w, w, w, S0))
    cs.append(XCase("heads", 2, 1, 17, 17, 17, S0))
    cs.append(XCase("heads", 1, 32, 16, 16, 16, S0))
    cs.append(XCase("map", 2, 3, 32, 16, 16, S0))             # Hs = 2w, Ws = w
    cs.append(XCase("map", 1, 2, 15, 45, 15, S0))             # Hs = w, Ws = 3w
    cs.append(XCase("scale", 2, 3, 17, 17, 17, 0.25))
    return cs


XL_CASES = _xl_cases()
MANY_CASE = XCase("many", 2, 2, 48, 96, 16, S0)              # 36 windows x 2 heads x 2 query blocks: workgroups loop, partials sum


def xid(c):
    return f"{c.group}-w{c.w}-{c.Hs}x{c.Ws}-H{c.H}-B{c.B}-scale{c.scale:.4f}"


def np_of(c):
    return 32 * ((c.w * c.w + 31) // 32)


class XlOperands:
    """qkv (B, L, 3, H, 32) and dout (B, L, H*32) bf16; table ((2w-1)^2, H) fp32, nonzero; mix = None.  q, k, v, do: the fp64
    views (B, L, H, 32).  The attributes of attn_mix_ref.WindowOperands."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(SEED + 32452843 + 7919 * (XL_CASES + [MANY_CASE]).index(c))
        L = c.Hs * c.Ws
        self.case = c
        self.geometry = (c.Hs, c.Ws, c.w, 0, 0)
        self.qkv = (torch.randn((c.B, L, 3, c.H, 32), generator=g)).bfloat16()
        self.dout = (torch.randn((c.B, L, c.H * 32), generator=g)).bfloat16()
        self.table = 0.3 * torch.randn((2 * c.w - 1) ** 2, c.H, generator=g)
        self.mix = None
        self.q, self.k, self.v = (self.qkv[:, :, i].double() for i in range(3))
        self.do = self.dout.double().view(c.B, L, c.H, 32)


@lru_cache(maxsize=None)
def xl_operands(c):
    return XlOperands(c)


# ---- the operation, per window ------------------------------------------------------------------------------------------------
def _windows_of(o, idx=None):
    c = o.case
    N = c.w * c.w
    qs = scaled_bf16(o.q, c.scale)                                                     # L1: the operand IS bf16(s q)
    qw, kw, vw, dw = (to_windows(t, o.geometry) for t in (qs, o.k, o.v, o.do))
    idx = relative_position_index(c.w) if idx is None else idx
    bias = o.table.double()[idx.view(-1)].view(N, N, c.H).permute(2, 0, 1)
    return qw, kw, vw, dw, bias, idx


def xl_reference(o, fault=None):
    """-> dict: out (B, L, H, 32), lse / delta (B nW, H, N), dq / dk / dv (B, L, H, 32), dT ((2w-1)^2, H), all fp64."""
    assert fault is None or fault in XL_FAULTS
    c = o.case
    N, NP, NU = c.w * c.w, np_of(c), (2 * c.w - 1) ** 2
    idx = relative_position_index(c.w)
    if fault == "rel_off_by_one_row":
        idx = (idx + (2 * c.w - 1)) % NU
    qs, k, v, do, bias, idx = _windows_of(o, idx)
    s = c.scale
    S = (s * qs if fault == "scale_twice" else qs) @ k.transpose(-2, -1) + bias.unsqueeze(0)
    if fault == "padding_counted" and NP > N:
        # the padded keys as the kernels stage them — zero rows with the table coordinates of the last real token — with their
        # logits left in the softmax
        pad = bias[:, :, N - 1:N].unsqueeze(0).expand(S.shape[0], -1, -1, NP - N)
        lse = torch.logsumexp(torch.cat([S, pad], -1), -1)
    else:
        lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse.unsqueeze(-1))
    dP = do @ v.transpose(-2, -1)
    PdP = P * dP
    delta = (PdP[..., :NP - 32] if fault == "delta_misses_a_tile" else PdP).sum(-1)
    dS = P * (dP - delta.unsqueeze(-1))
    r = dict(out=P @ v, dq=s * (dS @ k) * (s if fault == "scale_twice" else 1.0), dk=dS.transpose(-2, -1) @ qs, dv=P.transpose(-2, -1) @ do)
    res = {n: from_windows(r[n], o.geometry) for n in ("out", "dq", "dk", "dv")}
    res["lse"], res["delta"] = lse, delta
    per_pair = dS.sum(0)
    res["dT"] = _dtable(c, idx, per_pair.transpose(-2, -1) if fault == "dT_wrong_diagonal" else per_pair)
    return res


def xl_model(o, rounded=True, garbage=None):
    """The kernels' arithmetic with (rounded=True) or without their bf16 roundings, in the layout of xl_reference.
    `garbage`: a float — the key side is padded to NP rows as the kernels see it, with k = v = garbage in the rows past N and the
    kernels' rule applied (S = -inf, P = 0 there); the result must not depend on it."""
    c = o.case
    N, NP = c.w * c.w, np_of(c)
    qw, kw, vw, dw, bias, idx = _windows_of(o)
    mask = torch.zeros(qw.shape[0], N, N, dtype=torch.float64)
    if garbage is not None and NP > N:
        G, H = qw.shape[:2]
        fill = torch.full((G, H, NP - N, 32), float(garbage), dtype=torch.float64)
        kw, vw = torch.cat([kw, fill], 2), torch.cat([vw, fill], 2)
        bias = torch.cat([bias, bias[:, :, N - 1:N].expand(-1, -1, NP - N)], 2)
        mask = torch.cat([mask, torch.full((G, N, NP - N), float("-inf"), dtype=torch.float64)], 2)
    r = _core(qw, kw, vw, dw, c.scale, bias, mask, bf16 if rounded else ident)
    res = {n: from_windows(r[n][:, :, :N], o.geometry) for n in ("out", "dq", "dk", "dv")}
    res["lse"], res["delta"] = r["lse"], r["delta"]
    res["dT"] = _dtable(c, idx, r["dS"][..., :N].sum(0))
    return res


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def _bound(r, qs, k, v, do, s, bias, NP):
    D = qs.shape[-1]
    NT = NP // 32
    u = U32
    P = r["P"]
    T = lambda x: x.transpose(-2, -1)                                # noqa: E731
    A_S = qs.abs() @ T(k.abs()) + bias.abs().unsqueeze(0)
    e_S = (D + 2) * u * A_S
    alse = r["lse"].abs().unsqueeze(-1)
    e_lse = (P * e_S).sum(-1, keepdim=True) + u * (alse + NP / 2 + 5 * NT + 34)
    E_P = P * (e_S + e_lse + 2 * u * (A_S + alse) + 2 * u) + TINY
    A_dP = do.abs() @ T(v.abs())
    E_dP = D * u * A_dP
    A_dl = (P * A_dP).sum(-1, keepdim=True)
    E_dl = (E_P * A_dP + P * E_dP).sum(-1, keepdim=True) + (NP / 2 + 2) * u * A_dl
    A_dS = P * (A_dP + A_dl)
    E_dS = E_P * (A_dP + A_dl) + P * (E_dP + E_dl) + 2 * u * A_dS
    h_P, h_dS = hu(P + E_P) + E_P, hu(r["dS"].abs() + E_dS) + E_dS                          # rounded operand + its fp32 error

    def stored(ref, rest):
        return rest + hu(ref.abs() + rest)

    b = {"lse": e_lse.squeeze(-1), "delta": E_dl.squeeze(-1)}
    b["out"] = stored(r["out"], h_P @ v.abs() + NP * u * (P @ v.abs()))
    b["dv"] = stored(r["dv"], T(h_P) @ do.abs() + NP * u * (T(P) @ do.abs()))
    b["dk"] = stored(r["dk"], T(h_dS) @ qs.abs() + NP * u * (T(A_dS) @ qs.abs()))
    b["dq"] = stored(r["dq"], s * (h_dS @ k.abs() + NP * u * (A_dS @ k.abs())) + u * s * (A_dS @ k.abs()))
    b["E_dS"], b["A_dS"] = E_dS.sum(0), A_dS.sum(0)
    return b


@lru_cache(maxsize=None)
def xl_ref_and_bound(c):
    """-> (reference dict, bound dict) in the layout of xl_reference; computed once per case and shared."""
    o = xl_operands(c)
    qw, kw, vw, dw, bias, idx = _windows_of(o)
    N = c.w * c.w
    G = qw.shape[0]
    r = _core(qw, kw, vw, dw, c.scale, bias, torch.zeros(G, N, N, dtype=torch.float64), ident)
    b = _bound(r, qw, kw, vw, dw, c.scale, bias, np_of(c))
    bound = {n: from_windows(b[n], o.geometry) for n in ("out", "dq", "dk", "dv")}
    bound["lse"], bound["delta"] = b["lse"], b["delta"]
    pairs = torch.zeros((2 * c.w - 1) ** 2, dtype=torch.float64).index_add_(0, idx.view(-1), torch.ones(N * N, dtype=torch.float64))
    bound["dT"] = _dtable(c, idx, b["E_dS"]) + (G * pairs * U32).unsqueeze(1) * _dtable(c, idx, b["A_dS"])
    return xl_reference(o), bound
