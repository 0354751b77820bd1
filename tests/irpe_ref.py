"""fp64 reference, rounding model, per-element bound and the two case lists for the kernel-level tests of the fused iRPE
attention families: csrc/irpe_attn.hip (head_dim 64, <= 64 buckets, no mask: `irpe_fused.fwd_core` / `bwd_core`) and
csrc/irpe_attn_x.hip (head_dim 32 | 64, row width 64 | 128, key padding mask: `fwd_core_x` / `bwd_core_x`).

Same three pieces as tests/attn_mix_ref.py, whose `hu`, `bf16`, `scaled_bf16` and `worst_ratio` are used here as they are:
  * `reference` — fp64 autograd of the statement in the header of irpe_attn.hip (:5-11, :33-37) on the bf16-rounded operands:
    contextual lookups on q, k and v, bias mode on q and k, a key padding mask (probability exactly 0 for a masked key, lse
    over the real keys), causal attention, attention dropout with the kernels' own keep mask (`irpe_fused.dropout_keep_mask`,
    `dropout_threshold`, scale float32(1) / (float32(1) - float32(p)) as `to_args` computes it).  Every tensor the kernels
    return: out, lse, delta, dq, dk, dv, the gradient of each table, and the side rows sv, lkg (= LK), gg (= G), dlk, dlq.
    `fault=` applies one deliberate error (tests/test_irpe_ref_cpu.py: each must break the bound).
  * `model` — the same arithmetic by hand with a bf16 rounding wherever the kernels have one (list below).
  * `ref_and_bound` — the reference and a bound per element, computed once per case and shared by the tests.

Rounding points (bf16, round to nearest even, `f2bf` attn_common.hpp:43).  b = irpe_attn.hip, x = irpe_attn_x.hip, l = attn_lane.hpp.
  R1  bf16(s q) as the operand of every score product: `scaled` l:25-30 at b:302, b:520, x:296, x:498; `scaled_raw` l:31 at b:760,
      x:730 (the query tiles of the key launch).  Exact for s = 2^-k.
  R2  the fp32 tables as bf16 MFMA operands: `stage_table_T` b:121-126 / `stage_table_R` b:128-133 (Wk b:310, b:534, b:637; Wq
      b:312, b:668, b:742, b:845; Wv b:426, b:535); `stage_T` x:94-99 / `stage_R` x:101-106 (x:306, x:308, x:410, x:513-514, x:608,
      x:640, x:712, x:815).  Bias tables: `bias_rows_to_lds` b:198-204, x:200-206.
  R3  the lookup rows kept as bf16: LK = bf16((s q) Wk) `lookups_to_lds` b:193-194 / x:196 (forward b:319 / x:315; backward b:549 /
      x:525, copied bit for bit to `lkg` b:552 / x:528 and read by the key launch b:762 / x:732); G = bf16(dO Wv^T) b:555 / x:531
      (`gg` b:557 / x:533); LQ = bf16(s (k Wq)) — the product of the UNSCALED k, times s in fp32, then rounded: `lq_tile` b:259 /
      x:239 (forward), `irpe_lq_rows_kernel` b:674 / x:646 (query launch) and the key launch's own keys b:749 / x:719 — one
      form in all three places (see "Scale").
  R4  P through `from_acc` before P V: b:405 / x:392, at the UNNORMALISED scale exp(A - m), m the lazy running maximum (b:368-372 /
      x:358-361); the dropout factor is applied first (b:397 / x:387).
  R5  P (normalised, dropped) through `from_acc` before P^T dO: b:826 / x:795.
  R6  dS through `from_acc` before dS k (b:620 / x:592) and before dS^T (s q) (b:827 / x:796).
  R7  the bucket sums SV (fp32 scatter-add of the UNROUNDED dropped P, times 1 / l) as a bf16 row: `srow_frag` l:121-126 at b:443 /
      x:428 — both the `sv` row and the operand of SV Wv.
  R8  the bucket gradients dLK / dLQ (fp32 scatter-add of the UNROUNDED dS) as bf16 rows: `srow_frag` at b:645 / x:616 (`dlk` and
      the operand of dLK Wk^T) and b:853 / x:823 (`dlq`); the operand of dLQ Wq^T is bf16(s dLQ) (b:855 / x:825).
  R9  the table-gradient kernels (b:881-914, x:851-902) round NOTHING: their operands are bf16 already (q, k raw; the dlk, dlq, sv
      rows; dO), the accumulation is fp32, the factor s is applied in fp32 at the end (b:913 / x:899).  Bias mode sums the bf16
      rows in fp32 (irpe_fused.py, `bias_grad`).
  R10 the bf16 stores (`store_row` l:129-144) of out (b:449 / x:434), dq after the fp32 multiplication by s (b:654 / x:625), dk, dv
      (b:864-865 / x:834-835).
  R11 delta = dO . bf16(out) in fp32 (b:522 / x:500): the STORED out.
  lse, delta and the table gradients never pass through bf16 themselves.

Bound.  As in attn_mix_ref.py: u = 2^-24, hu(x) = half an ulp of the bf16 grid at |x|, A(.) = the same formula with every factor
replaced by its absolute value.  The deterministic roundings R2 and R3 are applied in the fp64 arithmetic the bound is built
around (`centre`: every other rounding off), and the bound is widened by the known shift |centre - ref| (the `y67` device
there).  A lookup row element whose fp32 error E(x) = D u A(x) reaches a rounding boundary (`flip`) is off by up to
E + 2 hu(|x| + E) and carries that into the logits (LK, LQ) or into dP (G); every other row element equals the centre's exactly,
bound 0.  Then, per
element, first order:
    e_S   = (D + 4) u A(S) + flips                        D products and additions, two dot2 additions of the lookups
    e_exp = 4 u (A(S) + |lse| + 8)                        exp2f (2 ulps), the fused multiply-add of its argument, m log2 e
    E(lse) = sum_j P (e_S + e_exp) + u (|lse| + NP + 4 NT + 64)      the row sum, one rescaling per tile at most, __logf of
                                                                    l in [1, NP e^8] (3 ulps of 16), m + log l
    E(P)  = P (e_S + E(lse) + e_exp) + 2^-126             exactly 0 for a masked key (a select in x, exp2(-inf) in b)
    P~ = keep P / (1 - p):  E = E(P) / (1 - p) + u P~
    out:  sum_j (2^-8 P~ + E(P~)) |v|                     R4 — the conversion happens at the scale exp(lse - m), which the bound does
                                                          not know: 2^-8 x is the supremum of hu(c x) / c over c
          + (NP + NT + 2) u A + SV term (R7: hu(SV + E) + E, E(SV) = scatter of E(P~) + (NP + NT + 2) u SV; W more roundings)
          + hu(|out| + rest)                              R10
    delta: sum_d |dO| bound(out) + (D + 2) u A            R11
    dP = dO . v + G:  E = (D + 4) u A + flips of G;  times keep / (1 - p): + u A
    dS = P (dP~ - delta): E = E(P) (A(dP~) + |delta|) + P (E(dP~) + E(delta)) + 2 u A(dS)
    dq, dk, dv: hu(x + E) + E of the rounded operand (R5, R6, R8) times the other factor, NP u A for the accumulation (W u A for
    the bucket contraction), one more for s, the store R10.  dlk / dlq rows: hu(x + E) + E, E = scatter of E(dS) + NP u A.
    table gradients: the row bounds times |s q| (|s k|, |dO|), plus (NP + B + H + 2) u A; bias mode: (B L + H) u A.
No constant is fitted to a GPU run.

Scale.  For s = 2^-k (every head_dim-64 model: 64^-0.5; the tests' 0.25 at head_dim 32) R1 is exact.  For head_dim 32's own
32^-0.5 it is a rounding of the operand, which the reference has too (the operand IS bf16(s q)); the table-gradient kernels use
q itself (R9), a known shift that the centre carries.  LQ has ONE form in the forward, the query launch and the key launch
(R3): bf16(s (k Wq)).  bf16(bf16(s k) Wq) is the same number for s = 2^-k and another one otherwise, and a key launch that had
it would recompute probabilities the saved lse does not belong to.  On ordinary operands the two differ by a rounding, below
the bf16 stores; `x-truescale-d32-lq-pin` (keys and table built so that k Wq cancels exactly, `Operands._term`) makes them
differ by tenths, and `model(..., key_lq_scaled_k=True)` shows on the CPU that the other form leaves the bound there.
"""
from collections import namedtuple
from functools import lru_cache
import math
import zlib

import numpy as np
import torch

from attn_mix_ref import TINY, U32, bf16, hu, ident, scaled_bf16, worst_ratio  # noqa: F401  (worst_ratio: for the tests)

SEED = 20241019

# ---- cases --------------------------------------------------------------------------------------------------------------------
# tq / tk / tv: None | ("syn", nb, mode, perhead) — ids drawn uniformly, a table of exactly nb buckets — | ("mod", method, mode,
# perhead) — a real irpe.iRPE / iRPE_Cross module, ratio 1.9.  mask: None | a kind of MASKS (image 0 unmasked).  layout (x only):
# "packed" slices of one tensor | "separate" buffers | "seqfirst".  hw: rectangular map (default: square, L - side^2 skipped tokens).
ICase = namedtuple("ICase", "tag fam B H L D tq tk tv scale drop causal mask layout hw")
MASKS = ("none", "last", "from32", "tile1", "allbut0", "allbutlast", "even")


def syn(nb, mode="ctx", perhead=False):
    return ("syn", nb, mode, perhead)


def mod(method, mode="ctx", perhead=False):
    return ("mod", method, mode, perhead)


def C(tag, fam, L, tq=None, tk=None, tv=None, B=2, H=3, D=64, scale=None, drop=0.0, causal=False, mask=None, layout="packed",
      hw=None):
    if scale is None:
        scale = 0.125 if D == 64 else 0.25
    return ICase(tag, fam, B, H, L, D, tq, tk, tv, scale, drop, causal, mask, layout, hw)


def _qkv(t):
    return dict(tq=t, tk=t, tv=t)


def _base_cases():
    cs = []
    s50 = syn(50)
    for L in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 257):
        cs.append(C(f"len-L{L}", "base", L, **_qkv(s50)))
    for bits in range(7):                                                          # (q + k + v at L = 65 is in the sweep above)
        cs.append(C("subset-" + ("".join(n for n, b in zip("qkv", (4, 2, 1)) if bits & b) or "none"), "base", 65,
                    tq=s50 if bits & 4 else None, tk=s50 if bits & 2 else None, tv=s50 if bits & 1 else None))
    for H in (1, 2, 5):
        cs.append(C(f"heads-perhead-H{H}", "base", 33, H=H, **_qkv(syn(50, perhead=True))))
    cs.append(C("heads-shared-H1", "base", 33, H=1, **_qkv(s50)))
    for B in (1, 3):
        cs.append(C(f"batch-B{B}", "base", 33, B=B, **_qkv(s50)))
    for nb in (1, 2, 51, 52, 63, 64):
        cs.append(C(f"nb{nb}-k", "base", 65, tk=syn(nb)))
        cs.append(C(f"nb{nb}-qkv", "base", 65, **_qkv(syn(nb))))
    for nb in (51, 52):
        cs.append(C(f"bias-q-nb{nb}", "base", 65, tq=syn(nb, "bias", True)))
        cs.append(C(f"bias-k-nb{nb}", "base", 65, tk=syn(nb, "bias", True)))
        cs.append(C(f"bias-qk-ctxv-nb{nb}", "base", 65, tq=syn(nb, "bias", True), tk=syn(nb, "bias", True), tv=syn(nb)))
    for L in (50, 37):                                                             # 7 x 7 + 1 and 6 x 6 + 1 tokens
        cs.append(C(f"mod-product-perhead-L{L}", "base", L, **_qkv(mod("product", perhead=True))))
        cs.append(C(f"mod-product-shared-L{L}", "base", L, **_qkv(mod("product"))))
        for method in ("euc", "quant", "cross"):
            cs.append(C(f"mod-{method}-L{L}", "base", L, **_qkv(mod(method))))
        cs.append(C(f"mod-cross-bias-L{L}", "base", L, tq=mod("cross", "bias", True), tk=mod("cross", "bias", True)))
    cs.append(C("mod-product-rect5x8", "base", 40, hw=(5, 8), **_qkv(mod("product", perhead=True))))
    for p in (0.1, 0.5):
        for L in (33, 129):
            cs.append(C(f"drop{p}-L{L}", "base", L, drop=p, **_qkv(s50)))
    cs.append(C("drop0.25-notable", "base", 65, drop=0.25))
    for L in (1, 32, 33, 77, 128, 129):
        cs.append(C(f"causal-L{L}", "base", L, causal=True))
    cs.append(C("causal-rpek", "base", 65, causal=True, tk=s50))
    cs.append(C("causal-drop", "base", 33, causal=True, drop=0.25))
    return cs


def _x_cases():
    cs = []
    full, thin = (1, 31, 32, 33, 64, 65, 128, 129), (32, 33, 128, 129)
    for L in full:
        cs.append(C(f"d32w64-qkv49-L{L}", "x", L, D=32, **_qkv(syn(49))))
        cs.append(C(f"d32w128-k81-L{L}", "x", L, D=32, tk=syn(81)))
        cs.append(C(f"d64w128-k82-L{L}", "x", L, D=64, tk=syn(82)))
        cs.append(C(f"d64w64-mask-qkv50-L{L}", "x", L, D=64, mask="last" if L > 1 else "none", **_qkv(syn(50))))
    for nb in (65, 127, 128):
        for L in thin:
            cs.append(C(f"d32w128-k{nb}-L{L}", "x", L, D=32, tk=syn(nb)))
    for kind, L in (("from32", 65), ("tile1", 96), ("allbut0", 65), ("allbutlast", 65), ("even", 65)):      # ("last": above)
        cs.append(C(f"pad-{kind}-L{L}", "x", L, mask=kind, **_qkv(syn(50))))
    cs.append(C("pad-from32-d32-k81", "x", 65, D=32, mask="from32", tk=syn(81)))
    for layout in ("seqfirst", "separate", "packed"):
        cs.append(C(f"layout-{layout}", "x", 65, D=32, mask="last", layout=layout, tk=syn(81, perhead=True)))
    cs.append(C("bias-k-w128", "x", 65, D=32, tk=syn(81, "bias", True)))
    for H in (1, 8):
        cs.append(C(f"heads-H{H}", "x", 33, D=32, H=H, tk=syn(81, perhead=True)))
    cs.append(C("drop-mask", "x", 65, drop=0.1, mask="even", **_qkv(syn(50))))
    cs.append(C("causal-mask", "x", 65, causal=True, mask="last", **_qkv(syn(50))))
    cs.append(C("truescale-d32-k81", "x", 65, D=32, scale=32 ** -0.5, mask="last", tk=syn(81)))
    cs.append(C("truescale-d32-qkv49", "x", 33, D=32, scale=32 ** -0.5, **_qkv(syn(49))))
    cs.append(C("truescale-d32-lq-pin", "x", 65, D=32, scale=32 ** -0.5, tq=("pin", 49, "ctx", False)))
    return cs


BASE_CASES = _base_cases()
X_CASES = _x_cases()


def cid(c):
    return f"{c.fam}-{c.tag}"


def row_width_of(c):
    """Width of the bucket-indexed side rows: 64, or 128 above 64 buckets (irpe_fused.row_width)."""
    nb = max([t.nb for t in operands(c).terms if t is not None], default=1)
    return 64 if nb <= 64 else 128


def padded_len(L):
    return (L + 31) // 32 * 32


# ---- operands -------------------------------------------------------------------------------------------------------------------
Term = namedtuple("Term", "table ids nb bias perhead module")       # table fp32 (H', D, nb) | (H', nb, D) | (H', nb); ids long (L, L)


def key_mask(kind, B, L):
    """(B, L) bool, True = the key takes no part; image 0 unmasked."""
    m = torch.zeros(B, L, dtype=torch.bool)
    j = torch.arange(L)
    row = {"none": j < 0, "last": j == L - 1, "from32": j >= 32, "tile1": (j >= 32) & (j < 64), "allbut0": j > 0,
           "allbutlast": j < L - 1, "even": j % 2 == 1}[kind]
    if B > 1:
        m[1] = row
    return m


class Operands:
    def __init__(self, c):
        seed = SEED + zlib.crc32(repr(c).encode())
        g = torch.Generator().manual_seed(seed)
        self.case = c
        B, H, L, D = c.B, c.H, c.L, c.D
        self.qkv = torch.randn((B, L, 3, H, D), generator=g).bfloat16()
        self.dout = torch.randn((B, L, H * D), generator=g).bfloat16()
        if c.tq is not None and c.tq[0] == "pin":            # every key a power of two times ONE vector (see _term)
            base = self.qkv[0, 0, 1, 0].clone()
            alpha = torch.tensor([0.5, 1.0, 2.0])[torch.arange(L) % 3].bfloat16()
            self.qkv[:, :, 1] = (alpha.view(1, L, 1, 1) * base.view(1, 1, 1, D)).expand(B, L, H, D)
        perm = lambda t: t.double().permute(0, 2, 1, 3)                              # noqa: E731  -> (B, H, L, D)
        self.q, self.k, self.v = (perm(self.qkv[:, :, i]) for i in range(3))
        self.do = perm(self.dout.view(B, L, H, D))
        self.terms = tuple(self._term(spec, which, g) for spec, which in zip((c.tq, c.tk, c.tv), "qkv"))
        assert len({t.nb for t in self.terms if t is not None}) <= 1, "one bucket count for all terms"
        self.pad = key_mask(c.mask, B, L) if c.mask is not None else None
        self.seed = seed % (2 ** 31 - 1)
        self.keepscale = None                                                        # (B, H, L, L): keep / (1 - p)
        if c.drop:
            from cream_amd.irpe_fused import dropout_keep_mask, dropout_threshold
            keep = torch.from_numpy(dropout_keep_mask(self.seed, B, H, L).astype(np.int64)) >= dropout_threshold(c.drop)
            self.keepscale = keep.double() * float(np.float32(1) / (np.float32(1) - np.float32(c.drop)))

    def _term(self, spec, which, g):
        if spec is None:
            return None
        c = self.case
        kind, a, mode, perhead = spec
        Hh = c.H if perhead else 1
        if kind == "syn":
            nb = a
            ids = torch.randint(0, nb, (c.L, c.L), generator=g)
            shape = (Hh, nb) if mode == "bias" else ((Hh, nb, c.D) if which == "v" else (Hh, c.D, nb))
            return Term(0.3 * torch.randn(shape, generator=g), ids, nb, mode == "bias", perhead, None)
        if kind == "pin":
            # rpe_q table whose every column is a power of two (up to 2^10) times a vector orthogonal to the keys' common vector
            # PAIR BY PAIR (w[2i] = k[2i+1], w[2i+1] = -k[2i]): k Wq is exactly 0 in any arithmetic whose products are exact, so
            # bf16(s (k Wq)) = 0, while bf16(s k) Wq keeps the rounding errors of s k times up to 2^10 — for a scale that is no
            # power of two the two forms of the lookup differ by tenths, not by a rounding
            assert which == "q" and mode == "ctx" and not perhead
            base = self.qkv[0, 0, 1, 0].float()
            perp = torch.stack((base[1::2], -base[0::2]), 1).flatten()
            cu = (2.0 ** (torch.arange(a) % 11)) * (1 - 2 * (torch.arange(a) % 2))
            return Term((perp[:, None] * cu[None, :]).unsqueeze(0).contiguous(), torch.randint(0, a, (c.L, c.L), generator=g), a,
                        False, False, None)
        from cream_amd.irpe import build_rpe, get_rpe_config, iRPE_Cross
        h, w = c.hw if c.hw is not None else (int(math.sqrt(c.L)),) * 2
        cfg = get_rpe_config(ratio=1.9, method=a, mode=mode, shared_head=not perhead, skip=c.L - h * w, rpe_on=which)
        m = build_rpe(cfg, head_dim=c.D, num_heads=c.H)["qkv".index(which)]
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
        hw = c.hw if c.hw is not None else (None, None)
        if type(m) is iRPE_Cross:
            ids, _, _, nb = m.merged_ids_for(c.L, "cpu", *hw)
            table = m.merged_table(c.L, "cpu", *hw).detach()
        else:
            ids, nb = m.bucket_ids_for(c.L, "cpu", *hw), m.num_buckets
            table = (m.lookup_table_bias if mode == "bias" else m.lookup_table_weight).detach()
        return Term(table.clone(), ids.long(), nb, mode == "bias", perhead, m)

    def valid(self, fault=None):
        """(B, 1, L, L) bool: key j takes part for query i."""
        c = self.case
        ok = torch.ones(c.B, 1, c.L, c.L, dtype=torch.bool)
        if self.pad is not None:
            pad = torch.roll(self.pad, 1, dims=1) if fault == "mask_off_by_one" else self.pad
            ok = ok & ~pad[:, None, None, :]
        if c.causal:
            i, j = torch.arange(c.L)[:, None], torch.arange(c.L)[None, :]
            tri = (j < i) | ((i == 0) & (j == 0)) if fault == "causal_strict" else j <= i
            ok = ok & tri
        return ok


@lru_cache(maxsize=None)
def operands(c):
    return Operands(c)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
FAULTS = ("idq_untransposed", "idk_idv_swapped", "head_stride0", "wv_transposed", "bucket_zeroed", "bias_wrong_side",
          "mask_off_by_one", "keep_not_on_sv", "tile_last_token", "causal_strict")
TABLES = ("dWq", "dWk", "dWv")


def fault_applies(fault, c):
    """Whether the deliberate error can change anything in this case (the reasons are in profiles/NOTES_irpe_kernel_tests.md)."""
    terms = (c.tq, c.tk, c.tv)
    nb = max([t[1] if t[0] != "mod" else 2 for t in terms if t is not None], default=0)
    any_t = any(t is not None for t in terms)
    live = c.tv is not None or (c.L > 1 and nb > 1)          # L = 1 or one bucket: dS sums to zero, d Wq = d Wk = 0 exactly
    tq = operands(c).terms[0]
    return {"idq_untransposed": c.tq is not None and not torch.equal(tq.ids, tq.ids.t()),     # (euclidean, quant: symmetric ids)
            "idk_idv_swapped": c.tk is not None and c.tv is not None and c.tk[0] == "syn" and c.L > 1 and nb > 1,
            "head_stride0": any(t is not None and t[3] for t in terms) and c.H > 1,
            "wv_transposed": c.tv is not None and nb > 1,
            "bucket_zeroed": any_t and live,
            "bias_wrong_side": any(t is not None and t[2] == "bias" for t in terms[:2]) and c.L > 1 and nb > 1,
            "mask_off_by_one": c.mask not in (None, "none") and c.B > 1,
            "keep_not_on_sv": bool(c.drop) and c.tv is not None,
            "tile_last_token": any_t and live and c.L >= 32,
            "causal_strict": c.causal and c.L > 1}[fault]


def _heads(W, t, H, stride0=False):
    """table (H', ...) -> (H, ...) as the head stride reads it."""
    if stride0 and t.perhead:
        return W[:1].expand(H, *W.shape[1:])
    return W.expand(H, *W.shape[1:])


def _scatter(x, ids, nb):
    """x (B, H, L, L), ids (L, L) -> (B, H, L, nb): sums of x[..., i, j] over the j with ids[i, j] = u."""
    B, H, L, _ = x.shape
    return torch.zeros(B, H, L, nb, dtype=x.dtype).scatter_add_(-1, ids.expand(B, H, L, L), x)


def _table_grads(o, s, qraw, kraw, do, rows, skip_token=None):
    """The three table gradients from the (bf16 or exact) rows, as the table-gradient kernels and `bias_grad` form them."""
    tq, tk, tv = o.terms
    res = {}
    sel = (lambda t: t) if skip_token is None else (lambda t: t[:, :, skip_token:skip_token + 1])
    for name, t, x, row in (("dWq", tq, kraw, rows.get("dlq")), ("dWk", tk, qraw, rows.get("dlk"))):
        if t is None:
            continue
        gpart = sel(row).sum((0, 2)) if t.bias else s * torch.einsum('bhid,bhiu->hdu', sel(x), sel(row))
        res[name] = gpart if t.perhead else gpart.sum(0, keepdim=True)
    if tv is not None:
        gpart = torch.einsum('bhiu,bhid->hud', sel(rows["sv"]), sel(do))
        res["dWv"] = gpart if tv.perhead else gpart.sum(0, keepdim=True)
    return res


RESIDUALS = ("rWq", "rWk", "rWv")


def residuals(o, t, kernel_form):
    """{rW*: d table - the table-gradient product of t's OWN side rows}: what the table-gradient kernels add to the rows they are
    handed.  kernel_form: q itself times s at the end (R9); otherwise the forward's operand bf16(s q) (autograd of the statement)."""
    s = o.case.scale
    part = _table_grads(o, s, o.q if kernel_form else scaled_bf16(o.q, s) / s, o.k, o.do, {n: t[n].double() for n in ("dlq", "dlk", "sv") if n in t})
    return {"r" + n[1:]: t[n].double() - part[n] for n in part}


def reference(o, fault=None):
    """fp64 autograd of the statement.  -> dict: out, dq, dk, dv (B, H, L, D); lse, delta (B, H, L); dWq / dWk / dWv in the
    tables' shapes; sv, lkg, gg, dlk, dlq (B, H, L, nb) — only those of the terms present."""
    assert fault is None or fault in FAULTS
    c = o.case
    B, H, L = c.B, c.H, c.L
    s = c.scale
    q, k, v = (t.clone().requires_grad_(True) for t in (o.q, o.k, o.v))
    sq = s * q
    qs = sq + (scaled_bf16(o.q, s) - sq).detach()            # the operand IS bf16(s q) (R1); exact for s = 2^-k
    ks = s * k
    tq, tk, tv = o.terms
    W = [t.table.double().clone().requires_grad_(True) if t is not None else None for t in o.terms]
    st0 = fault == "head_stride0"
    idq, idk, idv = (t.ids if t is not None else None for t in o.terms)
    if fault == "idk_idv_swapped":
        idk, idv = idv, idk
    S = qs @ k.transpose(-2, -1)
    LK = LQ = None
    if tk is not None:
        Wk = _heads(W[1], tk, H, st0)
        LK = Wk[None, :, None, :].expand(B, H, L, tk.nb) * 1.0 if tk.bias else torch.einsum('bhid,hdu->bhiu', qs, Wk)
        LK.retain_grad()
        idx = idk.t() if (fault == "bias_wrong_side" and tk.bias) else idk
        S = S + LK.gather(-1, idx.expand(B, H, L, L))
    if tq is not None:
        Wq = _heads(W[0], tq, H, st0)
        LQ = Wq[None, :, None, :].expand(B, H, L, tq.nb) * 1.0 if tq.bias else torch.einsum('bhjd,hdu->bhju', ks, Wq)
        LQ.retain_grad()
        idx = idq.t() if fault == "idq_untransposed" or (fault == "bias_wrong_side" and tq.bias) else idq
        S = S + LQ.gather(-1, idx.expand(B, H, L, L)).transpose(-2, -1)          # [i, j] = LQ[j, idq[j, i]]
    S = S.masked_fill(~o.valid(fault), float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = S.softmax(-1)
    P.retain_grad()
    Pd = P if o.keepscale is None else P * o.keepscale
    out = Pd @ v
    rows = {}
    if tv is not None:
        Wv = _heads(W[2], tv, H, st0)
        if fault == "wv_transposed":
            Wv = Wv.reshape(H, c.D, tv.nb).transpose(1, 2)
        SV = _scatter(P if fault == "keep_not_on_sv" else Pd, idv, tv.nb)
        out = out + torch.einsum('bhiu,hud->bhid', SV, Wv)
        rows["sv"] = SV.detach()
        rows["gg"] = torch.einsum('bhid,hud->bhiu', o.do, Wv.detach())
    (out * o.do).sum().backward()
    res = {"out": out.detach(), "lse": lse.detach(), "delta": (P * P.grad).sum(-1).detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    if tk is not None:
        rows["lkg"], rows["dlk"] = LK.detach(), LK.grad
        res["dWk"] = W[1].grad
    if tq is not None:
        rows["dlq"] = LQ.grad
        res["dWq"] = W[0].grad
    if tv is not None:
        res["dWv"] = W[2].grad
    res.update(rows)
    res = {n: t.clone() for n, t in res.items()}
    last = next((n for n in reversed(TABLES) if n in res), None)
    if fault == "bucket_zeroed" and last is not None:
        t = o.terms[TABLES.index(last)]
        axis = 1 if (last == "dWv" or t.bias) else 2
        cnt = torch.bincount(t.ids.flatten(), minlength=t.nb).double()
        dead = res[last].abs().amax([a for a in range(res[last].dim()) if a != axis]) == 0   # (every pair of the bucket masked)
        u = int(torch.where((cnt > 0) & ~dead, cnt, torch.full_like(cnt, float("inf"))).argmin())     # the least populated bucket
        res[last].select(axis, u).zero_()
    if fault == "tile_last_token" and last is not None:                         # token 31: the last of the first 32-tile
        part = _table_grads(o, s, scaled_bf16(o.q, s) / s, o.k, o.do, res, skip_token=31)
        res[last] = res[last] - part[last]
    res.update(residuals(o, res, False))
    return res


# ---- the arithmetic by hand, with the kernels' rounding points ----------------------------------------------------------------------
def lazy_max(S):
    """The forward's running maximum after the last tile (irpe_attn.hip:366-372): it moves to a tile's maximum only when that
    exceeds it by more than 8.  S (B, H, L, L) with -inf at masked keys -> (B, H, L)."""
    m = torch.full(S.shape[:-1], float("-inf"), dtype=S.dtype)
    for t0 in range(0, S.shape[-1], 32):
        tm = S[..., t0:t0 + 32].max(-1).values
        m = torch.where(tm > m + 8.0, tm, m)
    return m


def _core(o, rnd, rnd_lk=None, key_lq_scaled_k=False):
    """-> dict of every output and of the intermediates the bound needs.  rnd: the bf16 rounding (or the identity); rnd_lk: the
    one of R2 and R3 alone (default: rnd)."""
    c = o.case
    B, H, L = c.B, c.H, c.L
    s = c.scale
    rnd_lk = rnd_lk or rnd
    q, k, v, do = o.q, o.k, o.v, o.do
    qs = scaled_bf16(q, s)
    tq, tk, tv = o.terms
    T = lambda x: x.transpose(-2, -1)                                                  # noqa: E731
    r = {"qs": qs}
    S = qs @ T(k)
    if tk is not None:
        Wkb = rnd_lk(_heads(tk.table.double(), tk, H))                                 # R2
        xLK = Wkb[None, :, None, :].expand(B, H, L, tk.nb) if tk.bias else torch.einsum('bhid,hdu->bhiu', qs, Wkb)
        LK = rnd_lk(xLK)                                                               # R3
        gk = tk.ids.expand(B, H, L, L)
        S = S + LK.gather(-1, gk)
        r.update(Wkb=Wkb, xLK=xLK, LK=LK)
    if tq is not None:
        Wqb = rnd_lk(_heads(tq.table.double(), tq, H))
        xLQ = Wqb[None, :, None, :].expand(B, H, L, tq.nb) if tq.bias else s * torch.einsum('bhjd,hdu->bhju', k, Wqb)
        LQ = rnd_lk(xLQ)
        gq = tq.ids.expand(B, H, L, L)
        S = S + T(LQ.gather(-1, gq))
        r.update(Wqb=Wqb, xLQ=xLQ, LQ=LQ)
    ok = o.valid()
    S = S.masked_fill(~ok, float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse.unsqueeze(-1))
    Pd = P if o.keepscale is None else P * o.keepscale
    if rnd is ident:
        Pf = Pd
    else:                                                                              # R4: at the scale exp(A - m)
        cc = torch.exp(lse - lazy_max(S)).unsqueeze(-1)
        Pf = rnd(Pd * cc) / cc
    acc = Pf @ v
    if tv is not None:
        Wvb = rnd_lk(_heads(tv.table.double(), tv, H))                                 # (H, nb, D)
        gv = tv.ids.expand(B, H, L, L)
        SV = _scatter(Pd, tv.ids, tv.nb)
        SVb = rnd(SV)                                                                  # R7
        acc = acc + torch.einsum('bhiu,hud->bhid', SVb, Wvb)
        xG = torch.einsum('bhid,hud->bhiu', do, Wvb)
        G = rnd_lk(xG)                                                                 # R3
        r.update(Wvb=Wvb, SV=SV, sv=SVb, xG=xG, gg=G)
    out = rnd(acc)                                                                     # R10
    delta = (do * out).sum(-1)                                                         # R11
    dP = do @ T(v)
    if tv is not None:
        dP = dP + G.gather(-1, gv)
    dpr = dP if o.keepscale is None else dP * o.keepscale
    dS = P * (dpr - delta.unsqueeze(-1))
    dSb = rnd(dS)                                                                      # R6
    dqa = dSb @ k
    Pk, dSk = Pd, dS                                                                   # the key launch's own P and dS
    if key_lq_scaled_k:                                                                # its lookups as bf16(bf16(s k) Wq): NOT what the
        LQk = rnd_lk(torch.einsum('bhjd,hdu->bhju', scaled_bf16(k, s), Wqb))           # kernels do (test_irpe_ref_cpu.py)
        Pk = torch.exp((S - T(LQ.gather(-1, gq)) + T(LQk.gather(-1, gq))).masked_fill(~ok, float("-inf")) - lse.unsqueeze(-1))
        dSk = Pk * (dpr - delta.unsqueeze(-1))
        Pk = Pk if o.keepscale is None else Pk * o.keepscale
    dka = T(dSb if dSk is dS else rnd(dSk)) @ qs
    if tk is not None:
        dLK = _scatter(dS, tk.ids, tk.nb)
        dLKb = rnd(dLK)                                                                # R8
        if not tk.bias:
            dqa = dqa + torch.einsum('bhiu,hdu->bhid', dLKb, Wkb)
        r.update(dLK=dLK, dlk=dLKb, lkg=LK)
    if tq is not None:
        dLQ = _scatter(T(dSk), tq.ids, tq.nb)
        if not tq.bias:
            dka = dka + torch.einsum('bhju,hdu->bhjd', rnd(s * dLQ), Wqb)
        r.update(dLQ=dLQ, dlq=rnd(dLQ))
    # R9: the table-gradient kernels take q and k themselves and multiply by s in fp32; with every rounding off the operand is
    # the forward's bf16(s q) (the same number for s = 2^-k), so that this equals the autograd of the forward
    r.update(_table_grads(o, s, q if rnd_lk is not ident else qs / s, k, do, r))
    r.update(S=S, ok=ok, P=P, Pd=Pd, dP=dP, dS=dS, out=out, lse=lse, delta=delta, dq=rnd(s * dqa), dk=rnd(dka),
             dv=rnd(T(rnd(Pk)) @ do))                                                  # R5
    return r


OUTPUTS = ("out", "lse", "delta", "dq", "dk", "dv", "dWq", "dWk", "dWv", "sv", "lkg", "gg", "dlk", "dlq")


def _pack(o, r, kernel_form):
    res = {n: r[n] for n in OUTPUTS if n in r}
    res.update(residuals(o, res, kernel_form))
    return res


def model(o, rounded=True, key_lq_scaled_k=False):
    """The kernels' arithmetic with (rounded=True) or without their bf16 roundings, in the layout of `reference`.
    key_lq_scaled_k: the key launch with its rpe_q lookups formed from bf16(s k) — the form the kernels must not have."""
    return _pack(o, _core(o, bf16 if rounded else ident, key_lq_scaled_k=key_lq_scaled_k), rounded)


# ---- the bound -------------------------------------------------------------------------------------------------------------------
def _flip(x, E):
    """Error of a bf16 row element whose fp32 value y is within E of x: 0 where no rounding boundary lies inside [x - E, x + E]
    (both round to the same number), else |bf16(y) - bf16(x)| <= |y - x| + hu(y) + hu(x) <= E + 2 hu(|x| + E)."""
    return torch.where(bf16(x - E) != bf16(x + E), E + 2 * hu(x.abs() + E), torch.zeros_like(x))


def _bound(o, r):
    """Per-element bounds around the centre r = _core(o, ident, bf16) (module docstring)."""
    c = o.case
    B, H, L, D = c.B, c.H, c.L, c.D
    u, s = U32, c.scale
    NP = padded_len(L)
    NT, Wd = NP // 32, row_width_of(c)
    q, k, v, do, qs = o.q, o.k, o.v, o.do, r["qs"]
    tq, tk, tv = o.terms
    T = lambda x: x.transpose(-2, -1)                                                  # noqa: E731
    ok, P, Pd = r["ok"], r["P"], r["Pd"]
    ksc = o.keepscale if o.keepscale is not None else 1.0
    zero = torch.zeros_like(P)
    b = {}
    A_S, e_fl = qs.abs() @ T(k.abs()), zero
    if tk is not None:
        gk = tk.ids.expand(B, H, L, L)
        e_LK = torch.zeros_like(r["LK"]) if tk.bias else _flip(r["xLK"], D * u * torch.einsum('bhid,hdu->bhiu', qs.abs(), r["Wkb"].abs()))
        A_S, e_fl = A_S + r["LK"].abs().gather(-1, gk), e_fl + e_LK.gather(-1, gk)
        b["lkg"] = e_LK
    if tq is not None:
        gq = tq.ids.expand(B, H, L, L)
        e_LQ = torch.zeros_like(r["LQ"]) if tq.bias else \
            _flip(r["xLQ"], (D + 1) * u * s * torch.einsum('bhjd,hdu->bhju', k.abs(), r["Wqb"].abs()))
        A_S, e_fl = A_S + T(r["LQ"].abs().gather(-1, gq)), e_fl + T(e_LQ.gather(-1, gq))
    A_S = torch.where(ok, A_S, zero)
    e_S = torch.where(ok, (D + 4) * u * A_S + e_fl, zero)
    alse = r["lse"].abs().unsqueeze(-1)
    e_exp = 4 * u * (A_S + alse + 8)
    e_lse = (P * (e_S + e_exp)).sum(-1, keepdim=True) + u * (alse + NP + 4 * NT + 64)
    E_P = torch.where(ok, P * (e_S + e_lse + e_exp) + TINY, zero)
    E_Pd = E_P * ksc + u * Pd
    b["lse"] = e_lse.squeeze(-1)

    def stored(ref, rest):
        return rest + hu(ref.abs() + rest)

    # forward
    n_acc = (NP + NT + 2) * u
    rest = (2.0 ** -8 * Pd + E_Pd) @ v.abs() + n_acc * (Pd @ v.abs())
    if tv is not None:
        gv = tv.ids.expand(B, H, L, L)
        aWv = r["Wvb"].abs()
        E_SV = _scatter(E_Pd, tv.ids, tv.nb) + n_acc * r["SV"]
        h_SV = hu(r["SV"] + E_SV) + E_SV
        rest = rest + torch.einsum('bhiu,hud->bhid', h_SV, aWv) + Wd * u * torch.einsum('bhiu,hud->bhid', r["SV"], aWv)
        b["sv"] = h_SV
    b["out"] = stored(r["out"], rest)
    # backward
    E_dl = (do.abs() * b["out"]).sum(-1) + (D + 2) * u * (do.abs() * r["out"].abs()).sum(-1)
    b["delta"] = E_dl
    A_dP = do.abs() @ T(v.abs())
    E_dP = (D + 4) * u * A_dP
    if tv is not None:
        e_G = _flip(r["xG"], D * u * torch.einsum('bhid,hud->bhiu', do.abs(), aWv))
        A_dP = A_dP + r["gg"].abs().gather(-1, gv)
        E_dP = (D + 4) * u * A_dP + e_G.gather(-1, gv)
        b["gg"] = e_G
    A_dpr, E_dpr = A_dP * ksc, E_dP * ksc + u * A_dP * ksc
    adl = (r["delta"].abs() + E_dl).unsqueeze(-1)
    A_dS = P * (A_dpr + adl)
    E_dS = E_P * (A_dpr + adl) + P * (E_dpr + E_dl.unsqueeze(-1)) + 2 * u * A_dS
    h_dS = torch.where(ok, hu(r["dS"].abs() + E_dS) + E_dS, zero)
    h_Pb = torch.where(ok, hu(Pd + E_Pd) + E_Pd, zero)
    b["dv"] = stored(r["dv"], T(h_Pb) @ do.abs() + NP * u * (T(Pd) @ do.abs()))
    rest_q, slack_q = h_dS @ k.abs() + NP * u * (A_dS @ k.abs()), A_dS @ k.abs()
    rest_k = T(h_dS) @ qs.abs() + NP * u * (T(A_dS) @ qs.abs())
    rows = {}
    if tk is not None:
        A_dLK = _scatter(A_dS, tk.ids, tk.nb)
        E_dLK = _scatter(E_dS, tk.ids, tk.nb) + NP * u * A_dLK
        h_dLK = hu(r["dLK"].abs() + E_dLK) + E_dLK
        b["dlk"], rows["dlk"], rows["A_dlk"] = h_dLK, h_dLK, A_dLK
        if not tk.bias:
            aWk = r["Wkb"].abs()
            rest_q = rest_q + torch.einsum('bhiu,hdu->bhid', h_dLK, aWk) + Wd * u * torch.einsum('bhiu,hdu->bhid', A_dLK, aWk)
            slack_q = slack_q + torch.einsum('bhiu,hdu->bhid', A_dLK, aWk)
    if tq is not None:
        A_dLQ = _scatter(T(A_dS), tq.ids, tq.nb)
        E_dLQ = _scatter(T(E_dS), tq.ids, tq.nb) + NP * u * A_dLQ
        h_dLQ = hu(r["dLQ"].abs() + E_dLQ) + E_dLQ
        b["dlq"], rows["dlq"], rows["A_dlq"] = h_dLQ, h_dLQ, A_dLQ
        if not tq.bias:
            aWq = r["Wqb"].abs()
            h_sdLQ = hu(s * (r["dLQ"].abs() + E_dLQ)) + s * E_dLQ                    # the operand is bf16(s dLQ)
            rest_k = rest_k + torch.einsum('bhju,hdu->bhjd', h_sdLQ, aWq) + (Wd + 1) * u * s * torch.einsum('bhju,hdu->bhjd', A_dLQ, aWq)
    b["dq"] = stored(r["dq"], s * rest_q + u * s * slack_q)
    b["dk"] = stored(r["dk"], rest_k)
    if tv is not None:
        rows["sv"], rows["A_sv"] = b["sv"], r["SV"]
    # table gradients: the row bounds through the products, plus the fp32 accumulation over tokens, images and heads
    n_ctx, n_bias = (NP + B + H + 2) * u, (B * L + H) * u
    main = _table_grads(o, s, q.abs(), k.abs(), do.abs(), rows)
    acc = _table_grads(o, s, q.abs(), k.abs(), do.abs(), {"dlq": rows.get("A_dlq"), "dlk": rows.get("A_dlk"), "sv": rows.get("A_sv")})
    # the residuals: the fp32 accumulation alone, over rows as large as the reference's plus their own bound
    big = _table_grads(o, s, q.abs(), k.abs(), do.abs(), {n: r[n].abs() + b[n] for n in ("dlq", "dlk", "sv") if n in b})
    for n, t in zip(TABLES, o.terms):
        if t is not None:
            b[n] = main[n] + (n_bias if t.bias else n_ctx) * acc[n]
            b["r" + n[1:]] = (n_bias if t.bias else n_ctx) * big[n]
    return b


@lru_cache(maxsize=None)
def centre_and_slack(c):
    """-> (the fp64 arithmetic with R2 and R3 alone, the bound around it): what is left of the bound without the known shift."""
    o = operands(c)
    r = _core(o, ident, bf16)                                # R2 and R3 in, every other rounding out
    return _pack(o, r, True), _bound(o, r)


@lru_cache(maxsize=None)
def ref_and_bound(c):
    """-> (reference dict, bound dict), every tensor in the layout of `reference`; computed once per case and shared."""
    ref = reference(operands(c))
    centre, b = centre_and_slack(c)
    assert set(b) == set(ref) == set(centre), (sorted(b), sorted(ref))
    return ref, {n: b[n] + (centre[n] - ref[n]).abs() for n in ref}
