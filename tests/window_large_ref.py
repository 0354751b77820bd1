"""fp64 reference, rounding model, per-element bounds and the shared case list for the kernel-level tests of
csrc/window_attn_large.hip (fused window attention for windows of 9x9 .. 14x14, no head transforms).

The reference is `attn_mix_ref.window_reference` — the operation as the MODEL states it (a literal torch.roll,
window_partition, the `img_mask` of three slices per axis, the `relative_position_index` gather, softmax, P v, window_reverse,
the roll back; every gradient from fp64 autograd), with its injected faults.  It takes any operands object with the attributes
of `attn_mix_ref.WindowOperands`; `LargeOperands` is one.  Nothing in it follows the kernels' index arithmetic.

`large_model` is the same arithmetic written out by hand with a bf16 rounding at exactly the places where the kernels have one;
`large_ref_and_bound` is the reference together with a bound per output element, computed once per case and shared.

Rounding points (bf16, round to nearest even) of window_attn_large.hip:
  L1  `scaled()` on q: bf16(s q) (load_own with scale_it in the forward and launch Q; stage_rows with scale_a in launch K).
      Part of the semantics; exact for s = 2^-k.
  L2  `from_acc` on P before P v (rows_product in the forward's pass 2) and before P^T dO (launch K).
  L3  `from_acc` on dS before dS k (launch Q, pass B) and before dS^T (s q) (launch K).
  L4  the bf16 stores (store_row) of out, dq (after the fp32 multiplication by s), dk and dv.
  lse, delta and d table never pass through bf16 (fp32 registers, LDS and partials).

Bound.  u = 2^-24, hu(x) = half an ulp of the bf16 grid at |x|, A(.) = the formula with every factor replaced by its absolute
value, D = 32, NT = key tiles, NP = 32 NT.  Counts, step by step as the kernels compute:
    S = (s q).k + T + mask       D exact products, D additions, two more:               e_S = (D + 2) u A(S)
    lse = m + log(l)             pass 1 keeps (m, l) per lane over NT tiles: per tile 16 additions into `sum`, one multiplication
                                 of l by exp2f(..) (2 ulps) and one addition; the two lanes of a query are combined with two more
                                 multiplications by exp2f and one addition.  A term of l passes through at most
                                 16 + NT + 1 additions and NT + 1 multiplications by an exp2f of 2 ulps, its own exp2f (2 ulps) and
                                 the rounding of its argument — under NP / 2 + 5 NT + 10 roundings for every w here — then
                                 `__logf` on l in [1, NP] (3 ulps of log 224 = 5.5, under 17 u) and the rounding of m + log l:
                                 E(lse) = sum_j P e_S + u (|lse| + NP / 2 + 5 NT + 27)
    P = exp2f((S - lse) log2 e)  the logit error, the lse error, two roundings of a value of at most A(S) + |lse|, exp2f's
                                 2 ulps relative:  E(P) = P (e_S + E(lse) + 2 u (A(S) + |lse|) + 2 u) + 2^-126
                                 (2^-126: a probability behind the -100 mask underflows to 0 in fp32, as in attn_mix_ref)
    dP = dO . v                  E = D u A(dP)
    delta = sum_j P dP           two chains of fused multiply-adds of NP / 2 terms each, one addition of the chains and one across
                                 the lane pair: E = sum_j (E(P) A(dP) + P E(dP)) + (NP / 2 + 2) u A(delta)
    dS = P (dP - delta)          E = E(P) (A(dP) + A(delta)) + P (E(dP) + E(delta)) + 2 u A(dS)
    out, dv, dk, dq              the rounded operand (L2 / L3): hu(|a| + E(a)) + E(a) per term, NP fp32 additions of the
                                 contraction, dq one more for the multiplication by s, then the store (L4): hu(|ref| + rest)
    d table[u, h]                the fp32 errors of its (window, i, j) pairs plus one rounding per pair summed, whatever the
                                 order (a thread's chain per key tile, then onto the workgroup's entry, then the caller's sum
                                 of the partials: every term passes through at most `pairs` additions)
First-order throughout, as in attn_mix_ref.  No constant is fitted.
"""
from collections import namedtuple
from functools import lru_cache

import torch

from attn_mix_ref import (SEED, TINY, U32, bf16, from_windows, hu, ident, img_mask, relative_position_index, scaled_bf16,
                          to_windows, window_reference, worst_ratio)  # noqa: F401  (worst_ratio: for the tests)

LCase = namedtuple("LCase", "group B H Hs Ws w shift ms mixed scale")

LARGE_FAULTS = ("swap_dydx", "mask_for_shift", "dT_corner_zeroed", "roll_one_axis", "last_head_copied")


def _large_cases():
    cs = []
    for w in range(9, 15):                                   # NT = 3 (17 real keys in the last tile) .. 7 (4 real keys)
        cs.append(LCase("size", 2, 3, 2 * w, 3 * w, w, w // 2, w // 2, False, 0.25))
    for H in (1, 3, 5, 32):
        cs.append(LCase("heads", 1, H, 28, 28, 14, 7, 7, False, 0.25))
    w = 12
    for shift, ms in ((0, 0), (1, 1), (w - 1, w - 1), (0, w // 2), (w // 2, 0)):
        cs.append(LCase("shift", 1, 2, 24, 36, w, shift, ms, False, 0.25))
    for shift, ms in ((0, 0), (7, 7)):                       # a single window; with the mask, whole buckets are masked
        cs.append(LCase("single", 3, 3, 14, 14, 14, shift, ms, False, 0.25))
    cs.append(LCase("scale", 2, 3, 28, 28, 14, 7, 7, False, 32 ** -0.5))
    return cs


LARGE_CASES = _large_cases()
MANY_CASE = LCase("many", 40, 2, 28, 28, 14, 7, 7, False, 0.25)   # 160 windows x 2 heads: workgroups loop, partials sum


def lid(c):
    return f"{c.group}-w{c.w}-{c.Hs}x{c.Ws}-s{c.shift}m{c.ms}-H{c.H}-B{c.B}-scale{c.scale:.4f}"


def np_of(c):
    return 32 * ((c.w * c.w + 31) // 32)


class LargeOperands:
    """qkv (B, L, 3, H, 32) and dout (B, L, H*32) bf16; table ((2w-1)^2, H) fp32; mix = None.  q, k, v, do: the fp64 views
    (B, L, H, 32).  The attributes of attn_mix_ref.WindowOperands."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(SEED + 15485863 + 7919 * (LARGE_CASES + [MANY_CASE]).index(c))
        L = c.Hs * c.Ws
        self.case = c
        self.geometry = (c.Hs, c.Ws, c.w, c.shift, c.ms)
        self.qkv = (torch.randn((c.B, L, 3, c.H, 32), generator=g)).bfloat16()
        self.dout = (torch.randn((c.B, L, c.H * 32), generator=g)).bfloat16()
        self.table = 0.3 * torch.randn((2 * c.w - 1) ** 2, c.H, generator=g)
        self.mix = None
        self.q, self.k, self.v = (self.qkv[:, :, i].double() for i in range(3))
        self.do = self.dout.double().view(c.B, L, c.H, 32)


@lru_cache(maxsize=None)
def large_operands(c):
    return LargeOperands(c)


# ---- the kernels' arithmetic, by hand ----------------------------------------------------------------------------------------
def _windows_of(o):
    c = o.case
    N = c.w * c.w
    qs = scaled_bf16(o.q, c.scale)                                                     # L1
    qw, kw, vw, dw = (to_windows(t, o.geometry) for t in (qs, o.k, o.v, o.do))
    idx = relative_position_index(c.w)
    bias = o.table.double()[idx.view(-1)].view(N, N, c.H).permute(2, 0, 1)
    mask = img_mask(c.Hs, c.Ws, c.w, c.ms).repeat(c.B, 1, 1)
    return qw, kw, vw, dw, bias, mask, idx


def _core(qs, k, v, do, s, bias, mask, rnd):
    """(G, H, N, D) fp64 per window; bias (H, N, N), mask (G, N, N); rnd: the bf16 rounding or the identity."""
    S = qs @ k.transpose(-2, -1) + bias.unsqueeze(0) + mask.unsqueeze(1)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse.unsqueeze(-1))
    Pb = rnd(P)                                                                        # L2
    dP = do @ v.transpose(-2, -1)
    delta = (P * dP).sum(-1)
    dS = P * (dP - delta.unsqueeze(-1))
    dSb = rnd(dS)                                                                      # L3
    return dict(S=S, P=P, dP=dP, dS=dS, lse=lse, delta=delta, out=rnd(Pb @ v), dq=rnd(s * (dSb @ k)),
                dk=rnd(dSb.transpose(-2, -1) @ qs), dv=rnd(Pb.transpose(-2, -1) @ do))     # L4


def _dtable(c, idx, per_pair):
    """(H, N, N) summed over the windows -> ((2w-1)^2, H): the bucket sums."""
    N = c.w * c.w
    return torch.zeros((2 * c.w - 1) ** 2, c.H, dtype=torch.float64).index_add_(
        0, idx.view(-1), per_pair.permute(1, 2, 0).reshape(N * N, c.H))


def large_model(o, rounded=True):
    """The kernels' arithmetic with (rounded=True) or without their bf16 roundings, in the layout of window_reference."""
    c = o.case
    qw, kw, vw, dw, bias, mask, idx = _windows_of(o)
    r = _core(qw, kw, vw, dw, c.scale, bias, mask, bf16 if rounded else ident)
    res = {n: from_windows(r[n], o.geometry) for n in ("out", "dq", "dk", "dv")}
    res["lse"], res["delta"] = r["lse"], r["delta"]
    res["dT"] = _dtable(c, idx, r["dS"].sum(0))
    return res


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def _bound(r, qs, k, v, do, s, bias, mask, NP):
    D = qs.shape[-1]
    NT = NP // 32
    u = U32
    P = r["P"]
    T = lambda x: x.transpose(-2, -1)                                # noqa: E731
    A_S = qs.abs() @ T(k.abs()) + bias.abs().unsqueeze(0) + mask.abs().unsqueeze(1)
    e_S = (D + 2) * u * A_S
    alse = r["lse"].abs().unsqueeze(-1)
    e_lse = (P * e_S).sum(-1, keepdim=True) + u * (alse + NP / 2 + 5 * NT + 27)
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
def large_ref_and_bound(c):
    """-> (reference dict, bound dict) in the layout of window_reference; computed once per case and shared."""
    o = large_operands(c)
    qw, kw, vw, dw, bias, mask, idx = _windows_of(o)
    r = _core(qw, kw, vw, dw, c.scale, bias, mask, ident)
    b = _bound(r, qw, kw, vw, dw, c.scale, bias, mask, np_of(c))
    bound = {n: from_windows(b[n], o.geometry) for n in ("out", "dq", "dk", "dv")}
    bound["lse"], bound["delta"] = b["lse"], b["delta"]
    N = c.w * c.w
    G = qw.shape[0]
    pairs = torch.zeros((2 * c.w - 1) ** 2, dtype=torch.float64).index_add_(0, idx.view(-1), torch.ones(N * N, dtype=torch.float64))
    bound["dT"] = _dtable(c, idx, b["E_dS"]) + (G * pairs * U32).unsqueeze(1) * _dtable(c, idx, b["A_dS"])
    return window_reference(o), bound
