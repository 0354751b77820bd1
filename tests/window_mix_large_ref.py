"""fp64 reference, rounding model, per-element bounds and the shared case list for the kernel-level tests of
csrc/window_attn_mix_large.hip (fused head-mixing window attention for windows of 9x9 .. 12x12, 1 <= H <= 16).

The reference is `attn_mix_ref.window_reference` — the operation as the MODEL states it (a literal torch.roll,
window_partition, the `img_mask` of three slices per axis, the `relative_position_index` gather, the two linears over heads,
softmax, P' v, window_reverse, the roll back; every gradient from fp64 autograd), with its injected faults.  It is generic in w
and takes any operands object with the attributes of `attn_mix_ref.WindowOperands`; `MixLargeOperands` is one (the class of
attn_mix_ref draws its seed from that file's own case list).  Nothing in it follows the kernels' index arithmetic.

`mix_large_model` is the same arithmetic written out by hand with a bf16 rounding at exactly the places where the kernels have
one; `mix_large_ref_and_bound` is the reference together with a bound per output element, computed once per case and shared.

Rounding points (bf16, round to nearest even) of window_attn_mix_large.hip:
  X1  `scaled()` on q: bf16(s q), attn_lane.hpp:26-31, used at window_attn_mix_large.hip:171 (own_scores: the forward's two
      passes and launch Q's two passes), :99 called at :583 (stream_tile with scale_a, launch K) and :112 called at :634
      (stage_tile with scale_a, launch K).  Part of the semantics ("(s q)"); exact for s = 2^-k.
  X2  `from_acc` on P' before P' V: rows_product, :120, called at :325 (forward, pass 2).
  X3  `from_acc` on dS before dS k (:120 called at :480, launch Q, pass B) and before dS^T (s q) (:120 called at :635, launch K).
  X4  `from_acc` on P' before P'^T dO: :120 called at :611 (launch K).
  X5  the bf16 stores (store_row, attn_lane.hpp:140-145) of out (:332), dq (:514, after the fp32 multiplication by s), dk and dv
      (:643-644).
  lse, delta, d table, d Wl, d bl, d Ww, d bw never pass through bf16 (fp32 registers, LDS and partials).

Bound.  u = 2^-24, hu(x) = half an ulp of the bf16 grid at |x|, A(.) = the formula with every factor replaced by its absolute
value, D = 32, NT = key tiles, NP = 32 NT.  The chain is that of attn_mix_ref (its docstring has the derivation of every line);
what the two-pass softmax over 3 to 5 tiles changes:
    S' = Wl S + bl + mask        as there: e_S' = (D + H + 2) u A(S')
    lse = m + log(l)             pass 1 keeps (m, l) per lane over NT tiles.  A term of l is exp2f((S' - mn) log2 e): exp2f's
                                 2 ulps and the two roundings of its argument, whose P-weighted mean is at most
                                 u (lse - sum_j P S') <= u log NP each (the row's entropy).  It then passes through additions —
                                 16 in its tile's chain, one per later tile, one across the lane pair: at most NP, whatever the
                                 order — and through at most NT + 1 multiplications by a rescaling exp2f((m - mn) log2 e) (the
                                 product's rounding, exp2f's 2 ulps, and its argument's rounding, which weighs at most
                                 x e^-x <= 1 on what it rescales: 4 each).  `__logf` on l in [1, NP]: 3 ulps of log NP, an ulp
                                 being at most 2 u |x|.  The rounding of m + log l: u |lse|.
                                 E(lse) = sum_j P e_S' + u (|lse| + NP + 8 log NP + 4 (NT + 1) + 2)
    P = exp2f((S' - lse) log2 e) the logit error, the lse error, two roundings of a value of at most A(S') + |lse|, exp2f's
                                 2 ulps relative:  E(P) = P (e_S' + E(lse) + 2 u (A(S') + |lse|) + 2 u) + 2^-126
    delta = sum_j P dP           two chains of fused multiply-adds of NP / 4 terms each per lane (8 per tile), one addition of the
                                 chains and one across the lane pair: (NP / 4 + 2) u A(delta) on top of the operands' errors
    d Wl, d bl, d Ww, d bw       a term passes through at most 22 + NT + items additions, items = windows x query tiles, as in
                                 attn_mix_ref (16 in its lane's chain over a tile, one per key tile into the lane's running
                                 share, 6 butterfly steps, one per work item into the workgroup's partial, one per workgroup)
    d table[u, h]                the fp32 errors of its (window, i, j) pairs plus one rounding per pair summed, whatever the
                                 order (a thread's additions onto the workgroup's entry item by item, then the caller's sum
                                 of the partials: every term passes through at most windows x pairs additions)
Everything else (P', dP', dP, dS', dS, the contractions over NP padded keys or queries, the stores) has the counts of
attn_mix_ref.  First-order throughout.  No constant is fitted.
"""
from functools import lru_cache
import math

import torch

from attn_mix_ref import (SEED, TINY, U32, WCase, WINDOW_FAULTS, _mix_fp64, _mix_params, bf16, from_windows, hu, ident, img_mask,  # noqa: F401
                          nt_of, relative_position_index, scaled_bf16, to_windows, window_reference, worst_ratio)

MIN_WINDOW, MAX_WINDOW, MAX_HEADS = 9, 12, 16              # the range of the kernels (32 heads are refused)


def _cases():
    cs = []
    for w in range(9, 13):                                   # key tiles 3, 4, 4, 5; padding 15, 28, 7, 16 keys
        cs.append(WCase("size", 2, 3, 2 * w, 3 * w, w, w // 2, w // 2, True, 0.25))
    for H in (1, 4, 5, 8, 9, 13, 16):                        # head slots 1 1 2 2 3 4 4; 5, 9, 13: an empty last slot in waves 1-3
        cs.append(WCase("heads", 2, H, 12, 12, 12, 0, 0, True, 0.25))
    w = 12
    for shift, ms in ((0, 0), (1, 1), (w - 1, w - 1), (0, w // 2), (w // 2, 0), (2, w - 2)):
        cs.append(WCase("shift", 1, 2, 24, 36, w, shift, ms, True, 0.25))
    for shift in (0, 6):                                     # a single window; with the mask, whole buckets are masked
        cs.append(WCase("single", 3, 3, 12, 12, 12, shift, 6, True, 0.25))
    cs.append(WCase("scale", 2, 3, 24, 24, 12, 6, 6, True, 32 ** -0.5))
    for w in (9, 10, 11):                                    # 2, 3 and 4 head slots at the other key-tile counts and padding tails
        for H in (5, 9, 16):
            cs.append(WCase("slots", 1, H, 2 * w, 2 * w, w, w // 2, w // 2, True, 0.25))
    return cs


MIX_LARGE_CASES = _cases()
# 16 windows x 5 query tiles = 80 work items: more than the 16 workgroups of a grid on 8 CUs (two per CU at 2 heads)
MANY_CASE = WCase("many", 4, 2, 24, 24, 12, 6, 6, True, 0.25)


def xid(c):
    return f"{c.group}-w{c.w}-{c.Hs}x{c.Ws}-s{c.shift}m{c.ms}-H{c.H}-B{c.B}-scale{c.scale:.4f}"


def np_of(c):
    return 32 * nt_of(c)


def slots_of(c):
    """Head slots per wave of the kernels' instantiation (dispatch, window_attn_mix_large.hip)."""
    return (c.H + 3) // 4


class MixLargeOperands:
    """qkv (B, L, 3, H, 32) and dout (B, L, H*32) bf16; table ((2w-1)^2, H), mix = (wl, bl, ww, bw) fp32.  q, k, v, do: the
    fp64 views (B, L, H, 32).  The attributes of attn_mix_ref.WindowOperands."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(SEED + 32452843 + 7919 * (MIX_LARGE_CASES + [MANY_CASE]).index(c))
        L = c.Hs * c.Ws
        self.case = c
        self.geometry = (c.Hs, c.Ws, c.w, c.shift, c.ms)
        self.qkv = torch.randn((c.B, L, 3, c.H, 32), generator=g).bfloat16()
        self.dout = torch.randn((c.B, L, c.H * 32), generator=g).bfloat16()
        self.table = 0.3 * torch.randn((2 * c.w - 1) ** 2, c.H, generator=g)
        self.mix = _mix_params(c.H, g)
        self.q, self.k, self.v = (self.qkv[:, :, i].double() for i in range(3))
        self.do = self.dout.double().view(c.B, L, c.H, 32)


@lru_cache(maxsize=None)
def mix_large_operands(c):
    return MixLargeOperands(c)


# ---- the kernels' arithmetic, by hand ----------------------------------------------------------------------------------------
def _windows_of(o):
    c = o.case
    N = c.w * c.w
    qs = scaled_bf16(o.q, c.scale)                                                     # X1
    qw, kw, vw, dw = (to_windows(t, o.geometry) for t in (qs, o.k, o.v, o.do))
    idx = relative_position_index(c.w)
    bias = o.table.double()[idx.view(-1)].view(N, N, c.H).permute(2, 0, 1)
    mask = img_mask(c.Hs, c.Ws, c.w, c.ms).repeat(c.B, 1, 1)
    return qw, kw, vw, dw, bias, mask, idx


def _core(qs, k, v, do, s, bias, mask, Wl, bl, Ww, bw, rnd):
    """(G, H, N, D) fp64 per window; bias (H, N, N), mask (G, N, N); rnd: the bf16 rounding or the identity."""
    H = qs.shape[1]
    S = qs @ k.transpose(-2, -1) + bias.unsqueeze(0)
    Sp = torch.einsum('oh,ghij->goij', Wl, S) + bl.view(1, H, 1, 1) + mask.unsqueeze(1)
    lse = torch.logsumexp(Sp, -1)
    P = torch.exp(Sp - lse.unsqueeze(-1))
    Pp = torch.einsum('oh,ghij->goij', Ww, P) + bw.view(1, H, 1, 1)
    Ppb = rnd(Pp)                                                                      # X2, X4
    dPp = do @ v.transpose(-2, -1)
    dP = torch.einsum('oh,goij->ghij', Ww, dPp)
    delta = (P * dP).sum(-1)
    dSp = P * (dP - delta.unsqueeze(-1))
    dS = torch.einsum('oh,goij->ghij', Wl, dSp)
    dSb = rnd(dS)                                                                      # X3
    return dict(S=S, P=P, Pp=Pp, dPp=dPp, dP=dP, dSp=dSp, dS=dS, lse=lse, delta=delta,
                out=rnd(Ppb @ v), dq=rnd(s * (dSb @ k)), dk=rnd(dSb.transpose(-2, -1) @ qs),          # X5
                dv=rnd(Ppb.transpose(-2, -1) @ do),
                dWl=torch.einsum('goij,ghij->oh', dSp, S), dbl=dSp.sum((0, 2, 3)),
                dWw=torch.einsum('goij,ghij->oh', dPp, P), dbw=dPp.sum((0, 2, 3)))


def _dtable(c, idx, per_pair):
    """(H, N, N) summed over the windows -> ((2w-1)^2, H): the bucket sums."""
    N = c.w * c.w
    return torch.zeros((2 * c.w - 1) ** 2, c.H, dtype=torch.float64).index_add_(
        0, idx.view(-1), per_pair.permute(1, 2, 0).reshape(N * N, c.H))


def mix_large_model(o, rounded=True):
    """The kernels' arithmetic with (rounded=True) or without their bf16 roundings, in the layout of window_reference."""
    c = o.case
    qw, kw, vw, dw, bias, mask, idx = _windows_of(o)
    r = _core(qw, kw, vw, dw, c.scale, bias, mask, *_mix_fp64(o), bf16 if rounded else ident)
    res = {n: from_windows(r[n], o.geometry) for n in ("out", "dq", "dk", "dv")}
    res.update({n: r[n] for n in ("lse", "delta", "dWl", "dbl", "dWw", "dbw")})
    res["dT"] = _dtable(c, idx, r["dS"].sum(0))
    return res


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def _bound(r, qs, k, v, do, s, bias, mask, Wl, bl, Ww, bw, NP):
    G, H, N, D = qs.shape
    NT = NP // 32
    u = U32
    aWl, aWw, P = Wl.abs(), Ww.abs(), r["P"]
    mixl = lambda W, x: torch.einsum('oh,ghij->goij', W, x)          # noqa: E731  rows: out
    mixt = lambda W, x: torch.einsum('oh,goij->ghij', W, x)          # noqa: E731  transposed
    T = lambda x: x.transpose(-2, -1)                                # noqa: E731
    A_S = qs.abs() @ T(k.abs()) + bias.abs().unsqueeze(0)
    A_Sp = mixl(aWl, A_S) + bl.abs().view(1, H, 1, 1) + mask.abs().unsqueeze(1)
    e_Sp = (D + H + 2) * u * A_Sp
    alse = r["lse"].abs().unsqueeze(-1)
    e_lse = (P * e_Sp).sum(-1, keepdim=True) + u * (alse + NP + 8 * math.log(NP) + 4 * (NT + 1) + 2)
    E_P = P * (e_Sp + e_lse + 2 * u * (A_Sp + alse) + 2 * u) + TINY
    A_Pp = mixl(aWw, P) + bw.abs().view(1, H, 1, 1)
    E_Pp = mixl(aWw, E_P) + (H + 1) * u * A_Pp
    A_dPp = do.abs() @ T(v.abs())
    E_dPp = D * u * A_dPp
    A_dP = mixt(aWw, A_dPp)
    E_dP = mixt(aWw, E_dPp) + H * u * A_dP
    A_dl = (P * A_dP).sum(-1, keepdim=True)
    E_dl = (E_P * A_dP + P * E_dP).sum(-1, keepdim=True) + (NP / 4 + 2) * u * A_dl
    A_dSp = P * (A_dP + A_dl)
    E_dSp = E_P * (A_dP + A_dl) + P * (E_dP + E_dl) + 2 * u * A_dSp
    A_dS = mixt(aWl, A_dSp)
    E_dS = mixt(aWl, E_dSp) + H * u * A_dS
    h_Pp, h_dS = hu(r["Pp"].abs() + E_Pp) + E_Pp, hu(r["dS"].abs() + E_dS) + E_dS          # rounded operand + its fp32 error

    def stored(ref, rest):
        return rest + hu(ref.abs() + rest)

    b = {"lse": e_lse.squeeze(-1), "delta": E_dl.squeeze(-1)}
    b["out"] = stored(r["out"], h_Pp @ v.abs() + NP * u * (A_Pp @ v.abs()))
    b["dv"] = stored(r["dv"], T(h_Pp) @ do.abs() + NP * u * (T(A_Pp) @ do.abs()))
    b["dk"] = stored(r["dk"], T(h_dS) @ qs.abs() + NP * u * (T(A_dS) @ qs.abs()))
    b["dq"] = stored(r["dq"], s * (h_dS @ k.abs() + NP * u * (A_dS @ k.abs())) + u * s * (A_dS @ k.abs()))
    n = 22 + NT + G * NT                                             # additions a term of an (H, H) or (H) gradient passes through
    b["E_dS"], b["A_dS"] = E_dS.sum(0), A_dS.sum(0)
    E_S = D * u * A_S
    b["dWl"] = torch.einsum('goij,ghij->oh', E_dSp, A_S) + torch.einsum('goij,ghij->oh', A_dSp, E_S) \
        + n * u * torch.einsum('goij,ghij->oh', A_dSp, A_S)
    b["dbl"] = E_dSp.sum((0, 2, 3)) + n * u * A_dSp.sum((0, 2, 3))
    b["dWw"] = torch.einsum('goij,ghij->oh', E_dPp, P) + torch.einsum('goij,ghij->oh', A_dPp, E_P) \
        + n * u * torch.einsum('goij,ghij->oh', A_dPp, P)
    b["dbw"] = E_dPp.sum((0, 2, 3)) + n * u * A_dPp.sum((0, 2, 3))
    return b


@lru_cache(maxsize=None)
def mix_large_ref_and_bound(c):
    """-> (reference dict, bound dict) in the layout of window_reference; computed once per case and shared."""
    o = mix_large_operands(c)
    qw, kw, vw, dw, bias, mask, idx = _windows_of(o)
    mix = _mix_fp64(o)
    r = _core(qw, kw, vw, dw, c.scale, bias, mask, *mix, ident)
    b = _bound(r, qw, kw, vw, dw, c.scale, bias, mask, *mix, np_of(c))
    bound = {n: from_windows(b[n], o.geometry) for n in ("out", "dq", "dk", "dv")}
    bound.update({n: b[n] for n in ("lse", "delta", "dWl", "dbl", "dWw", "dbw")})
    N = c.w * c.w
    G = qw.shape[0]
    pairs = torch.zeros((2 * c.w - 1) ** 2, dtype=torch.float64).index_add_(0, idx.view(-1), torch.ones(N * N, dtype=torch.float64))
    bound["dT"] = _dtable(c, idx, b["E_dS"]) + (G * pairs * U32).unsqueeze(1) * _dtable(c, idx, b["A_dS"])
    return window_reference(o), bound
