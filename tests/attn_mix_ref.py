"""fp64 references, rounding model, per-element bounds and the shared case lists for the kernel-level tests of the two
head-mixing attention families: csrc/window_attn.hip (Mini-Swin / Swin) and csrc/mini_attn.hip (Mini-DeiT).

Three functions per family, all on the CPU in fp64:
  * `window_reference` / `mini_reference` — the operation as the MODEL defines it (a literal torch.roll, window_partition, the
    `img_mask` of three slices per axis, the `relative_position_index` gather, the two linears over heads, softmax, P' v,
    window_reverse, the roll back; for Mini-DeiT the two 1x1 convolutions over heads and the contextual rpe on k gathered from a
    real iRPE module's bucket matrix), with every gradient from fp64 autograd of that same function.  Nothing in them follows
    the kernels' index arithmetic.  `fault=` applies one deliberate error (tests/test_attn_mix_ref_cpu.py: each must break the
    bound).
  * `window_model` / `mini_model` — the same arithmetic written out by hand (`_core`, the backward as the kernels' header
    comments state it) with a bf16 rounding at exactly the places where the kernels have one, and nowhere else (list below).
    With the rounding switched off it must agree with the autograd reference to fp64 noise (asserted by the CPU test).
  * `window_ref_and_bound` / `mini_ref_and_bound` — the reference together with a bound per output element, derived from those
    rounding points and from operation counts (`_core_bound`); computed once per case and shared by the tests.

Rounding points (bf16, round to nearest even).  window_attn.hip:
  W1  `scaled()` on q: bf16(s q), attn_lane.hpp:25-30, used at window_attn.hip:169 (own_scores), :97 / :577 (stream_tile with
      scale_a) and :110 / :638 (stage_tile with scale_a).  Part of the semantics ("(s q)" in the header); exact for s = 2^-k.
  W2  `from_acc` on P' before P' V: rows_product, window_attn.hip:118, called at :303.
  W3  `from_acc` on dS before dS k (:118 called at :474) and before dS^T (s q) (:118 called at :639).
  W4  `from_acc` on P' before P'^T dO: :118 called at :611.
  W5  the bf16 stores (store_row, attn_lane.hpp:139-144) of out (:311), dq (:507, after the fp32 multiplication by s), dk and
      dv (:647-648).
  lse, delta, d table, d Wl, d bl, d Ww, d bw never pass through bf16 (fp32 registers, LDS and partials).
mini_attn.hip has the same four (M1 `scaled` :77; M2 rows_product :117 called at :289; M3 :117 at :394 and :544; M4 :117 at
:522; M5 store_row :296, :436, :552-553) and, with rpe on k, four more:
  M6  the fp32 table Wk as a bf16 MFMA operand: lookups_to_lds :136-137 (forward, both backward query launches) and :432-433
      (dq += Wk dLK^T).
  M7  the lookup rows LK = (s q) Wk stored as bf16: :142-143 (LDS; copied bit for bit to `lkg` for the key launch, :202).
  M8  the bucket-gradient rows dLK (fp32 scatter-add of the UNROUNDED dS) converted to bf16, :430; that fragment is both the
      operand of dq += Wk dLK^T (:432-433) and the `dlk` row (:431) that cream_irpe_table_grad contracts with q
      (irpe_attn.hip:904-914: bf16 operands, fp32 accumulation, times s in fp32).

Bound.  u = 2^-24 (fp32), hu(x) = half an ulp of the bf16 grid at |x| = 2^(floor(log2 |x|) - 8): the largest error of ONE
round-to-nearest bf16 conversion of x (8 significant bits: the grid has 2^7 steps per binade).  hu(x) is 2^-9 |x| at the top
of a binade and 2^-8 |x| at its bottom; 2^-9 |ref| for a store would not be a bound — x = 1 + 2^-8 rounds with an error of
2^-8 — and the rounding model alone breaks it, so the store term is half an ulp, the exact figure.  A(.) is the same
formula with every factor replaced by its absolute value (the running error bound of a sum of products).  Per element:
    bound = hu(|ref| + rest)                                  for a bf16 store (W5 / M5), absent for fp32 outputs
          + rest,   rest = sum_j hu(|a_j| + E(a_j)) |b_j|     for every product with a rounded operand a (W2-W4, M2-M4, M8)
                         + sum_j E(a_j) |b_j| + K u A         the fp32 slack: the propagated fp32 error E of the operands plus
                                                              K roundings of the accumulation itself
The fp32 slack starts at the logits, element by element.  S_h = (s q).k + bias: D exact products, D additions.
S' = Wl S + bl + mask: H fused multiply-adds and two additions, so S'[i,j] is off by e_S' = (D + H + 2) u A(S')[i,j], with
A(S') = sum_h |Wl[o,h]| A(S_h) + |bl[o]| + |mask|.  (With rpe on k: see the end.)  The row's log-sum-exp moves by
the P-weighted mean of the logit errors; the kernels' lse = m + log(l) adds one rounding of m + log l, the row sum l (64
additions) and `__logf` on l in [1, 64] (3 ulps of log 64 = 4.2):
    E(lse) = sum_j P e_S' + u (|lse| + 80)                    (80 > 64 + 3 * 4.2 + the 2 ulps of exp2f)
which is the bound of lse itself.  A probability is exp2f((S' - lse) log2 e) (forward: (S' - m), then times 1 / l — the same
count): the logit error, the lse error, two roundings of a value of at most A(S') + |lse|, so
    E(P) = P (e_S' + E(lse) + 2 u (A(S') + |lse|)) + 2^-126
— the last term because fp32 has nothing below its smallest normal number that `exp2f` would return: a probability behind the
-100 mask is e^-100 = 4e-44 in the reference and 0 in the kernels, which is the whole value of a table bucket all of whose
(i, j) pairs are masked (a single-window map with a mask).  From there on every step adds its own count of roundings times its A:
    P' = Ww P + bw        E = sum_h |Ww| E(P_h) + (H + 1) u A(P')
    dP' = dO . v          E = D u A(dP')
    dP = Ww^T dP'         E = sum_o |Ww| E(dP'_o) + H u A(dP)
    delta = sum_j P dP    E = sum_j (E(P) A(dP) + P E(dP)) + (NP + 1) u A(delta)             NP = keys padded to 32
    dS' = P (dP - delta)  E = E(P) (A(dP) + A(delta)) + P (E(dP) + E(delta)) + 2 u A(dS')
    dS = Wl^T dS'         E = sum_o |Wl| E(dS'_o) + H u A(dS)
    out, dq, dk, dv: NP more (the contraction over the padded keys or queries); dq one more for the multiplication by s.
    d table[u, h]: one more per (window, i, j) pair of the bucket, whatever the order they are summed in.
    d Wl, d bl, d Ww, d bw: a term passes through at most 22 + NP / 32 + items additions, items = (windows or images) x query
    tiles: 16 in its lane's chain over a tile, one per key tile into the lane's running share, 6 butterfly steps across the
    wave, then one per work item into a workgroup's partial and one per workgroup in the caller's sum of the partials — for any
    grid at most `items` together.  (d Wl = sum dS'_o S_h also carries E(S_h) = D u A(S_h) + e_S.)
These are worst-case sums of absolute values.  Where a value is itself a heavily cancelling sum the bound is wide against the
value: d Wl (a covariance: the rows of dS' sum to zero) is held only to about its own size, i.e. against gross errors; d Ww
to about 1e-2, delta to 1e-3, a corner bucket of d table to 1e-2 (profiles/NOTES_attn_mix_tests.md has the figures).

rpe on k.  M6 and M7 perturb every logit by up to hu(LK) + sum_d |s q| hu(Wk), about 6e-3 per head and 3e-2 after Wl.  Carried
through the chain above as a worst case that term alone exceeds the gradients it bounds (every probability off by 3 %, no
cancellation anywhere).  But the two roundings are deterministic functions of the operands: the CPU knows bf16(Wk) exactly, and
LK = bf16(x), x = (s q) bf16(Wk), equals the kernels' row unless a rounding boundary lies within the fp32 error
E(x) = D u A(x) of the kernels' x — those elements are found (`flip`; a handful per case) and get e_S = 2 hu(x), every other
element e_S = 0.  So the bound of an rpe case is built around y67 = the fp64 arithmetic with M6 and M7 alone (every other
rounding off), exactly as above with that e_S and with M8 on top —
    E(dLK) = scatter of E(dS) + NP u A(dLK); d Wk: NP (tokens) + B (images) + H (heads of a shared table) additions more —
and is widened by the known shift: bound = |y67 - ref| + bound around y67.  It stays a bound around the fp64 reference of the
model's statement; |y67 - ref| is what the two roundings really do to this case's operands instead of what they could do at worst.
First-order throughout (products of two errors are dropped: they are below 2^-17 of the terms kept).  No constant is fitted.
"""
from collections import namedtuple
from functools import lru_cache
import math

import torch

U32 = 2.0 ** -24
TINY = 2.0 ** -126                                    # the smallest normal fp32 number
SEED = 20240607

# ---- case lists -------------------------------------------------------------------------------------------------------------
WCase = namedtuple("WCase", "group B H Hs Ws w shift ms mixed scale")
MCase = namedtuple("MCase", "group B H L rpe skip scale")       # rpe: None | 'shared' | 'perhead'


def _window_cases():
    cs = []
    for w in range(1, 9):                                    # NT = 1 (w <= 5), 4 real keys in tile 1 (w = 6), no padding (w = 8)
        for H, mixed in ((3, True), (5, False)):
            cs.append(WCase("size", 2, H, 2 * w, 3 * w, w, w // 2, w // 2, mixed, 0.25))
    for H in (1, 4, 5, 8, 9, 12, 13, 16):                    # HPW 1 1 2 2 3 3 4 4; 5, 9, 13: waves 1-3 with an empty last slot
        cs.append(WCase("heads", 2, H, 14, 14, 7, 3, 3, True, 0.25))
    for H in (1, 4, 5, 8, 9, 32):
        cs.append(WCase("heads", 2, H, 14, 14, 7, 3, 3, False, 0.25))
    for w, (Hs, Ws) in ((7, (14, 21)), (4, (8, 12))):
        for shift, ms in ((0, 0), (1, 1), (w - 1, w - 1), (0, w // 2), (w // 2, 0), (2, w - 2)):
            cs.append(WCase("shift", 2, 2, Hs, Ws, w, shift, ms, True, 0.25))
    for shift in (0, 3):
        cs.append(WCase("single", 3, 3, 7, 7, 7, shift, 3, True, 0.25))
    cs.append(WCase("scale", 2, 3, 14, 14, 7, 3, 3, True, 32 ** -0.5))
    return cs


def _mini_cases():
    cs = [MCase("heads", 2, H, 33, None, 0, 0.125) for H in (1, 4, 5, 8, 9, 12)]
    cs += [MCase("length", 2, H, L, None, 0, 0.125) for H in (5, 12) for L in (1, 2, 31, 32, 33, 63, 64, 65, 197)]
    for H, L in ((5, 36), (9, 37), (4, 196), (12, 197)):     # L = 37, 197: one leading token in the skip bucket
        side = int(math.sqrt(L))
        cs += [MCase("rpe", 2, H, L, kind, L - side * side, 0.125) for kind in ("shared", "perhead")]
    cs.append(MCase("scale", 2, 3, 33, None, 0, 64 ** -0.5))
    return cs


WINDOW_CASES = _window_cases()
MINI_CASES = _mini_cases()


def wid(c):
    return f"{c.group}-w{c.w}-{c.Hs}x{c.Ws}-s{c.shift}m{c.ms}-{'mix' if c.mixed else 'plain'}{c.H}-B{c.B}"


def mid(c):
    return f"{c.group}-H{c.H}-L{c.L}-{c.rpe or 'norpe'}{'-skip%d' % c.skip if c.rpe else ''}"


def hpw_of(c):
    """Head slots per wave of the window kernels' instantiation (dispatch, window_attn.hip: 1 without head transforms)."""
    return (c.H + 3) // 4 if c.mixed else 1


def nt_of(c):
    return (c.w * c.w + 31) // 32


# ---- small helpers ----------------------------------------------------------------------------------------------------------
def bf16(x):
    return x.float().bfloat16().double()


def ident(x):
    return x


def hu(x):
    """Half an ulp of the bf16 grid at |x| (0 at 0)."""
    m, e = torch.frexp(x.abs())                              # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 9))


def scaled_bf16(q, s):
    """`scaled()` of attn_lane.hpp bit for bit: the fp32 product of a bf16 value and the fp32 scale, converted to bf16."""
    return (q.float() * torch.tensor(s, dtype=torch.float32)).bfloat16().double()


def _normal_bf16(shape, g, std=1.0):
    return (std * torch.randn(shape, generator=g)).bfloat16()


def _mix_params(H, g):
    """eye + 0.3 randn (non-symmetric: [o,h] / [h,o] show), biases 0.2 randn — fp32, as the kernels read them."""
    wl = torch.eye(H) + 0.3 * torch.randn(H, H, generator=g)
    bl = 0.2 * torch.randn(H, generator=g)
    ww = torch.eye(H) + 0.3 * torch.randn(H, H, generator=g)
    bw = 0.2 * torch.randn(H, generator=g)
    return wl, bl, ww, bw


# ---- operands ---------------------------------------------------------------------------------------------------------------
class WindowOperands:
    """qkv (B, L, 3, H, 32) and dout (B, L, H*32) bf16; table ((2w-1)^2, H), wl, bl, ww, bw fp32 (mix = None without head
    transforms).  q, k, v, do: the fp64 views (B, L, H, 32)."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(SEED + 7919 * WINDOW_CASES.index(c))
        L = c.Hs * c.Ws
        self.case = c
        self.geometry = (c.Hs, c.Ws, c.w, c.shift, c.ms)
        self.qkv = _normal_bf16((c.B, L, 3, c.H, 32), g)
        self.dout = _normal_bf16((c.B, L, c.H * 32), g)
        self.table = 0.3 * torch.randn((2 * c.w - 1) ** 2, c.H, generator=g)
        self.mix = _mix_params(c.H, g) if c.mixed else None
        self.q, self.k, self.v = (self.qkv[:, :, i].double() for i in range(3))
        self.do = self.dout.double().view(c.B, L, c.H, 32)


class MiniOperands:
    """qkv (B, L, 3, H, 64) and dout (B, L, H*64) bf16; wl, ww (H, H, 1, 1) fp32; rpe: a real irpe.iRPE module (contextual,
    product method, transposed) with a std-0.3 table, or None."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(SEED + 104729 + 7919 * MINI_CASES.index(c))
        self.case = c
        self.qkv = _normal_bf16((c.B, c.L, 3, c.H, 64), g)
        self.dout = _normal_bf16((c.B, c.L, c.H * 64), g)
        wl, _, ww, _ = _mix_params(c.H, g)
        self.wl, self.ww = wl.reshape(c.H, c.H, 1, 1).contiguous(), ww.reshape(c.H, c.H, 1, 1).contiguous()
        self.rpe = None
        if c.rpe:
            from cream_amd.irpe import build_rpe, get_rpe_config
            cfg = get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=c.rpe == "shared", skip=c.skip, rpe_on='k')
            self.rpe = build_rpe(cfg, head_dim=64, num_heads=c.H)[1]
            with torch.no_grad():
                self.rpe.lookup_table_weight.copy_(0.3 * torch.randn(self.rpe.lookup_table_weight.shape, generator=g))
        self.q, self.k, self.v = (self.qkv[:, :, i].double() for i in range(3))
        self.do = self.dout.double().view(c.B, c.L, c.H, 64)


@lru_cache(maxsize=None)
def window_operands(c):
    return WindowOperands(c)


@lru_cache(maxsize=None)
def mini_operands(c):
    return MiniOperands(c)


# ---- the window geometry, as the model states it ------------------------------------------------------------------------------
def window_partition(x, w):
    """(B, Hs, Ws, C) -> (B nW, w, w, C), windows row-major."""
    B, Hs, Ws, C = x.shape
    return x.view(B, Hs // w, w, Ws // w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, w, w, C)


def window_reverse(xw, w, Hs, Ws):
    B = xw.shape[0] // ((Hs // w) * (Ws // w))
    return xw.view(B, Hs // w, Ws // w, w, w, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, Hs, Ws, -1)


def relative_position_index(w, swapped=False):
    ys, xs = torch.meshgrid(torch.arange(w), torch.arange(w), indexing="ij")
    ys, xs = ys.flatten(), xs.flatten()
    dy, dx = ys[:, None] - ys[None, :] + w - 1, xs[:, None] - xs[None, :] + w - 1
    if swapped:
        dy, dx = dx, dy
    return dy * (2 * w - 1) + dx


def img_mask(Hs, Ws, w, ms):
    """(nW, N, N) of {0, -100}: the `attn_mask` buffer of a block with shift_size = ms (zero without one)."""
    nW, N = (Hs // w) * (Ws // w), w * w
    if ms == 0:
        return torch.zeros(nW, N, N, dtype=torch.float64)
    img = torch.zeros(1, Hs, Ws, 1, dtype=torch.float64)
    n = 0
    for hs in (slice(0, -w), slice(-w, -ms), slice(-ms, None)):
        for ws in (slice(0, -w), slice(-w, -ms), slice(-ms, None)):
            img[:, hs, ws, :] = n
            n += 1
    ids = window_partition(img, w).view(-1, N)
    return torch.where(ids.unsqueeze(1) != ids.unsqueeze(2), -100.0, 0.0).double()


def to_windows(x, geometry, one_axis=False):
    """(B, L, H, D) of the unshifted map -> (B nW, H, N, D): roll(-shift), partition."""
    Hs, Ws, w, shift = geometry[:4]
    B, L, H, D = x.shape
    x = x.reshape(B, Hs, Ws, H * D)
    if shift > 0:
        x = torch.roll(x, shifts=(-shift,), dims=(1,)) if one_axis else torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    return window_partition(x, w).reshape(-1, w * w, H, D).permute(0, 2, 1, 3)


def from_windows(xw, geometry, one_axis=False):
    """(B nW, H, N, D) -> (B, L, H, D): reverse, roll(+shift)."""
    Hs, Ws, w, shift = geometry[:4]
    G, H, N, D = xw.shape
    x = window_reverse(xw.permute(0, 2, 1, 3).reshape(G, w, w, H * D), w, Hs, Ws)
    if shift > 0:
        x = torch.roll(x, shifts=(shift,), dims=(1,)) if one_axis else torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return x.reshape(-1, Hs * Ws, H, D)


def _mix_fp64(o):
    c = o.case
    if o.mix is None:
        eye = torch.eye(c.H, dtype=torch.float64)
        return eye, torch.zeros(c.H, dtype=torch.float64), eye.clone(), torch.zeros(c.H, dtype=torch.float64)
    return tuple(t.double() for t in o.mix)


WINDOW_FAULTS = ("swap_dydx", "wl_transposed", "bw_on_padded_keys", "mask_for_shift", "dT_corner_zeroed", "roll_one_axis",
                 "last_head_copied")
MINI_FAULTS = ("wl_transposed", "last_head_copied")


def _copy_last_head(res, names):
    for n, axis in names:
        t = res[n]
        if t.shape[axis] >= 2:
            t.select(axis, t.shape[axis] - 1).copy_(t.select(axis, t.shape[axis] - 2).clone())


def window_reference(o, fault=None):
    """fp64 autograd of the model's own statement.  -> dict: out (B, L, H, 32), lse / delta (B nW, H, N), dq / dk / dv
    (B, L, H, 32), dT, dWl, dbl, dWw, dbw (the last four absent without head transforms)."""
    assert fault is None or fault in WINDOW_FAULTS
    c = o.case
    Hs, Ws, w, shift, ms = o.geometry
    N, H = w * w, c.H
    q, k, v = (t.clone().requires_grad_(True) for t in (o.q, o.k, o.v))
    T = o.table.double().clone().requires_grad_(True)
    Wl, bl, Ww, bw = (t.clone().requires_grad_(True) for t in _mix_fp64(o))
    sq = c.scale * q
    qs = sq + (scaled_bf16(o.q, c.scale) - sq).detach()      # the operand IS bf16(s q) (W1); d qs / d q = s.  Exact for s = 2^-k
    one_axis = fault == "roll_one_axis"
    qw, kw, vw = (to_windows(t, o.geometry, one_axis) for t in (qs, k, v))
    attn = qw @ kw.transpose(-2, -1)
    idx = relative_position_index(w, swapped=fault == "swap_dydx")
    attn = attn + T[idx.view(-1)].view(N, N, H).permute(2, 0, 1).unsqueeze(0)
    if c.mixed:                                              # proj_l: nn.Linear(H, H) over the head axis
        attn = torch.einsum('oh,ghij->goij', Wl.t() if fault == "wl_transposed" else Wl, attn) + bl.view(1, H, 1, 1)
    mask = img_mask(Hs, Ws, w, shift if fault == "mask_for_shift" else ms)
    nW = mask.shape[0]
    attn = (attn.view(-1, nW, H, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, H, N, N)
    lse = torch.logsumexp(attn, -1)
    P = attn.softmax(-1)
    P.retain_grad()
    Pp = torch.einsum('oh,ghij->goij', Ww, P) + bw.view(1, H, 1, 1) if c.mixed else P
    x = Pp @ vw
    if fault == "bw_on_padded_keys" and c.mixed:             # the padded keys repeat the last real token
        x = x + (32 * nt_of(c) - N) * bw.view(1, H, 1, 1) * vw[:, :, N - 1:N, :]
    out = from_windows(x, o.geometry, one_axis)
    (out * o.do).sum().backward()
    res = {"out": out.detach(), "lse": lse.detach(), "delta": (P * P.grad).sum(-1).detach(),
           "dq": q.grad, "dk": k.grad, "dv": v.grad, "dT": T.grad}
    if c.mixed:
        res.update({"dWl": Wl.grad, "dbl": bl.grad, "dWw": Ww.grad, "dbw": bw.grad})
    res = {n: t.clone() for n, t in res.items()}
    if fault == "dT_corner_zeroed":
        res["dT"][0] = 0.0                                   # (dy, dx) = (-(w-1), -(w-1)): one (i, j) pair per window
    if fault == "last_head_copied":
        _copy_last_head(res, (("out", 2), ("dq", 2), ("dk", 2), ("dv", 2), ("lse", 1), ("delta", 1), ("dT", 1)))
    return res


def _rpe_terms(o):
    """(Wk (H', 64, nb) fp64, bucket ids (L, L) long) of the case's iRPE module, or None."""
    if o.rpe is None:
        return None
    return o.rpe.lookup_table_weight.detach().double(), o.rpe.bucket_ids_for(o.case.L, "cpu").long()


def mini_reference(o, fault=None):
    """fp64 autograd of MiniAttention's statement (mini_vision_transformer.py:84-114).  -> dict: out (B, L, H, 64), lse / delta
    (B, H, L), dq / dk / dv (B, L, H, 64), dWl, dWw (H, H), dWk (H', 64, nb) with rpe."""
    assert fault is None or fault in MINI_FAULTS
    c = o.case
    q, k, v = (t.clone().requires_grad_(True) for t in (o.q, o.k, o.v))
    Wl, Ww = (t.double().view(c.H, c.H).clone().requires_grad_(True) for t in (o.wl, o.ww))
    sq = c.scale * q
    qs = (sq + (scaled_bf16(o.q, c.scale) - sq).detach()).permute(0, 2, 1, 3)            # (B, H, L, 64)
    kh, vh = k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    attn = qs @ kh.transpose(-2, -1)
    Wk = None
    if o.rpe is not None:
        Wk, ids = _rpe_terms(o)
        Wk = Wk.clone().requires_grad_(True)
        lookup = qs @ (Wk[0] if Wk.shape[0] == 1 else Wk.unsqueeze(0))                 # (B, H, L, nb)
        attn = attn + lookup.gather(-1, ids.view(1, 1, c.L, c.L).expand(c.B, c.H, -1, -1))
    attn = torch.einsum('oh,bhij->boij', Wl.t() if fault == "wl_transposed" else Wl, attn)
    lse = torch.logsumexp(attn, -1)
    P = attn.softmax(-1)
    P.retain_grad()
    out = (torch.einsum('oh,bhij->boij', Ww, P) @ vh).permute(0, 2, 1, 3)
    (out * o.do).sum().backward()
    res = {"out": out.detach(), "lse": lse.detach(), "delta": (P * P.grad).sum(-1).detach(), "dq": q.grad, "dk": k.grad,
           "dv": v.grad, "dWl": Wl.grad, "dWw": Ww.grad}
    if Wk is not None:
        res["dWk"] = Wk.grad
    res = {n: t.clone() for n, t in res.items()}
    if fault == "last_head_copied":
        _copy_last_head(res, (("out", 2), ("dq", 2), ("dk", 2), ("dv", 2), ("lse", 1), ("delta", 1)))
    return res


# ---- the arithmetic by hand, with the kernels' rounding points ------------------------------------------------------------------
def _core(qs, k, v, do, s, bias, mask, Wl, bl, Ww, bw, rnd, rpe=None, rnd_lk=None):
    """All tensors (G, H, N, D) per group (window or image) in fp64; bias (H, N, N) or None, mask (G, N, N) or None, rpe =
    (Wk (H', D, nb), ids (N, N)) or None; rnd: the bf16 rounding (or the identity); rnd_lk: the one of M6 and M7 alone
    (default: rnd).  -> dict of the outputs and of every intermediate the bound needs."""
    G, H, N, D = qs.shape
    r = {}
    rnd_lk = rnd_lk or rnd
    S = qs @ k.transpose(-2, -1)
    if bias is not None:
        S = S + bias.unsqueeze(0)
    if rpe is not None:
        Wk, ids = rpe
        Wkb = rnd_lk(Wk).expand(H, -1, -1)                                             # M6
        idx = ids.view(1, 1, N, N).expand(G, H, -1, -1)
        LK = rnd_lk(torch.einsum('ghid,hdu->ghiu', qs, Wkb))                           # M7
        S = S + LK.gather(-1, idx)
        r["LK"] = LK
    Sp = torch.einsum('oh,ghij->goij', Wl, S) + bl.view(1, H, 1, 1)
    if mask is not None:
        Sp = Sp + mask.unsqueeze(1)
    lse = torch.logsumexp(Sp, -1)
    P = torch.exp(Sp - lse.unsqueeze(-1))
    Pp = torch.einsum('oh,ghij->goij', Ww, P) + bw.view(1, H, 1, 1)
    Ppb = rnd(Pp)                                                                      # W2, W4 / M2, M4
    out = rnd(Ppb @ v)                                                                 # W5 / M5
    dPp = do @ v.transpose(-2, -1)
    dP = torch.einsum('oh,goij->ghij', Ww, dPp)
    delta = (P * dP).sum(-1)
    dSp = P * (dP - delta.unsqueeze(-1))
    dS = torch.einsum('oh,goij->ghij', Wl, dSp)
    dSb = rnd(dS)                                                                      # W3 / M3
    dqa = dSb @ k
    if rpe is not None:
        dLK = torch.zeros(G, H, N, Wk.shape[-1], dtype=dS.dtype).scatter_add_(-1, idx, dS)      # of the unrounded dS
        dLKb = rnd(dLK)                                                                # M8
        dqa = dqa + torch.einsum('ghiu,hdu->ghid', dLKb, Wkb)
        dWk = s * torch.einsum('ghid,ghiu->hdu', qs / s if s != 0 else qs, dLKb)       # q itself, times s at the end
        r.update(dLK=dLK, dWk=dWk.sum(0, keepdim=True) if Wk.shape[0] == 1 else dWk)
    r.update(S=S, P=P, Pp=Pp, dPp=dPp, dP=dP, dSp=dSp, dS=dS, out=out, lse=lse, delta=delta,
             dq=rnd(s * dqa), dk=rnd(dSb.transpose(-2, -1) @ qs), dv=rnd(Ppb.transpose(-2, -1) @ do),
             dbias=dS.sum(0), dWl=torch.einsum('goij,ghij->oh', dSp, S), dbl=dSp.sum((0, 2, 3)),
             dWw=torch.einsum('goij,ghij->oh', dPp, P), dbw=dPp.sum((0, 2, 3)))
    return r


def _window_core(o, rnd):
    c = o.case
    Hs, Ws, w, shift, ms = o.geometry
    N = w * w
    qs = scaled_bf16(o.q, c.scale)
    qw, kw, vw, dw = (to_windows(t, o.geometry) for t in (qs, o.k, o.v, o.do))
    idx = relative_position_index(w)
    bias = o.table.double()[idx.view(-1)].view(N, N, c.H).permute(2, 0, 1)
    mask = img_mask(Hs, Ws, w, ms).repeat(c.B, 1, 1)
    return _core(qw, kw, vw, dw, c.scale, bias, mask, *_mix_fp64(o), rnd), idx


def _window_pack(o, r, idx):
    c = o.case
    N = c.w * c.w
    res = {n: from_windows(r[n], o.geometry) for n in ("out", "dq", "dk", "dv")}
    res["lse"], res["delta"] = r["lse"], r["delta"]
    res["dT"] = torch.zeros((2 * c.w - 1) ** 2, c.H, dtype=torch.float64).index_add_(
        0, idx.view(-1), r["dbias"].permute(1, 2, 0).reshape(N * N, c.H))
    if c.mixed:
        res.update({n: r[n] for n in ("dWl", "dbl", "dWw", "dbw")})
    return res


def window_model(o, rounded=True):
    """The kernels' arithmetic with (rounded=True) or without their bf16 roundings, in the layout of window_reference."""
    r, idx = _window_core(o, bf16 if rounded else ident)
    return _window_pack(o, r, idx)


def _mini_core(o, rnd, rnd_lk=None):
    c = o.case
    qs = scaled_bf16(o.q, c.scale)
    perm = lambda t: t.permute(0, 2, 1, 3)                   # noqa: E731
    zero = torch.zeros(c.H, dtype=torch.float64)
    return _core(perm(qs), perm(o.k), perm(o.v), perm(o.do), c.scale, None, None, o.wl.double().view(c.H, c.H), zero,
                 o.ww.double().view(c.H, c.H), zero, rnd, _rpe_terms(o), rnd_lk)


def _mini_pack(o, r):
    res = {n: r[n].permute(0, 2, 1, 3) for n in ("out", "dq", "dk", "dv")}
    res.update({n: r[n] for n in ("lse", "delta", "dWl", "dWw")})
    if o.rpe is not None:
        res["dWk"] = r["dWk"]
    return res


def mini_model(o, rounded=True):
    return _mini_pack(o, _mini_core(o, bf16 if rounded else ident))


# ---- the bound ----------------------------------------------------------------------------------------------------------------
def _core_bound(r, qs, k, v, do, s, bias, mask, Wl, bl, Ww, bw, Hm, rpe=None):
    """Per-element bounds of _core's outputs from the UNROUNDED intermediates r (module docstring).  Hm: the number of mix terms
    (H, or 0 without head transforms)."""
    G, H, N, D = qs.shape
    NP = 32 * ((N + 31) // 32)
    u = U32
    aWl, aWw, P = Wl.abs(), Ww.abs(), r["P"]
    mixl = lambda W, x: torch.einsum('oh,ghij->goij', W, x)          # noqa: E731  rows: out
    mixt = lambda W, x: torch.einsum('oh,goij->ghij', W, x)          # noqa: E731  transposed
    A_S = qs.abs() @ k.abs().transpose(-2, -1)
    if bias is not None:
        A_S = A_S + bias.abs().unsqueeze(0)
    e_S = None
    if rpe is not None:
        Wk, ids = rpe
        Wke = bf16(Wk).expand(H, -1, -1)                                                   # r holds M6 and M7 already
        idx = ids.view(1, 1, N, N).expand(G, H, -1, -1)
        x = torch.einsum('ghid,hdu->ghiu', qs, Wke)                                        # LK before M7
        E_x = D * u * torch.einsum('ghid,hdu->ghiu', qs.abs(), Wke.abs())
        assert torch.equal(bf16(x), r["LK"])
        flip = bf16(x - E_x) != bf16(x + E_x)                                              # a rounding boundary within the fp32 error
        A_S = A_S + r["LK"].abs().gather(-1, idx)
        e_S = torch.where(flip, 2 * hu(x.abs() + E_x), torch.zeros_like(x)).gather(-1, idx)
    A_Sp = mixl(aWl, A_S) + bl.abs().view(1, H, 1, 1)
    if mask is not None:
        A_Sp = A_Sp + mask.abs().unsqueeze(1)
    e_Sp = (D + Hm + 2) * u * A_Sp                                   # the logit S'[i,j] as the kernels hold it
    if e_S is not None:
        e_Sp = e_Sp + mixl(aWl, e_S)
    alse = r["lse"].abs().unsqueeze(-1)
    e_lse = (P * e_Sp).sum(-1, keepdim=True) + u * (alse + 80)       # the row's log-sum-exp
    E_P = P * (e_Sp + e_lse + 2 * u * (A_Sp + alse)) + TINY
    A_Pp = mixl(aWw, P) + bw.abs().view(1, H, 1, 1)
    E_Pp = mixl(aWw, E_P) + (Hm + 1) * u * A_Pp
    A_dPp = do.abs() @ v.abs().transpose(-2, -1)
    E_dPp = D * u * A_dPp
    A_dP = mixt(aWw, A_dPp)
    E_dP = mixt(aWw, E_dPp) + Hm * u * A_dP
    A_dl = (P * A_dP).sum(-1, keepdim=True)
    E_dl = (E_P * A_dP + P * E_dP).sum(-1, keepdim=True) + (NP + 1) * u * A_dl
    A_dSp = P * (A_dP + A_dl)
    E_dSp = E_P * (A_dP + A_dl) + P * (E_dP + E_dl) + 2 * u * A_dSp
    A_dS = mixt(aWl, A_dSp)
    E_dS = mixt(aWl, E_dSp) + Hm * u * A_dS
    h_Pp, h_dS = hu(r["Pp"].abs() + E_Pp) + E_Pp, hu(r["dS"].abs() + E_dS) + E_dS          # rounded operand + its fp32 error
    T = lambda x: x.transpose(-2, -1)                                # noqa: E731

    def stored(ref, rest):
        return rest + hu(ref.abs() + rest)

    b = {"lse": e_lse.squeeze(-1), "delta": E_dl.squeeze(-1)}
    b["out"] = stored(r["out"], h_Pp @ v.abs() + NP * u * (A_Pp @ v.abs()))
    b["dv"] = stored(r["dv"], T(h_Pp) @ do.abs() + NP * u * (T(A_Pp) @ do.abs()))
    b["dk"] = stored(r["dk"], T(h_dS) @ qs.abs() + NP * u * (T(A_dS) @ qs.abs()))
    rest_q = h_dS @ k.abs() + NP * u * (A_dS @ k.abs())
    if rpe is not None:
        A_dLK = torch.zeros_like(r["dLK"]).scatter_add_(-1, idx, A_dS)
        E_dLK = torch.zeros_like(r["dLK"]).scatter_add_(-1, idx, E_dS) + NP * u * A_dLK
        h_dLK = hu(r["dLK"].abs() + E_dLK) + E_dLK                                         # M8
        rest_q = rest_q + torch.einsum('ghiu,hdu->ghid', h_dLK, Wke.abs()) \
            + Wk.shape[-1] * u * torch.einsum('ghiu,hdu->ghid', A_dLK, Wke.abs())
        n = NP + G + (H if Wk.shape[0] == 1 else 0)                                        # tokens, then images, then heads
        bWk = torch.einsum('ghid,ghiu->hdu', qs.abs(), h_dLK) + (n + 1) * u * torch.einsum('ghid,ghiu->hdu', qs.abs(), A_dLK)
        b["dWk"] = bWk.sum(0, keepdim=True) if Wk.shape[0] == 1 else bWk
    b["dq"] = stored(r["dq"], s * rest_q + u * s * (A_dS @ k.abs()))
    n = 22 + NP // 32 + G * (NP // 32)                               # additions a term of an (H, H) or (H) gradient passes through
    b["dbias"] = E_dS.sum(0) + G * u * A_dS.sum(0)                                         # per (h, i, j): G terms
    b["A_dbias"] = A_dS.sum(0)
    E_S = D * u * A_S if e_S is None else D * u * A_S + e_S
    b["dWl"] = torch.einsum('goij,ghij->oh', E_dSp, A_S) + torch.einsum('goij,ghij->oh', A_dSp, E_S) \
        + n * u * torch.einsum('goij,ghij->oh', A_dSp, A_S)
    b["dbl"] = E_dSp.sum((0, 2, 3)) + n * u * A_dSp.sum((0, 2, 3))
    b["dWw"] = torch.einsum('goij,ghij->oh', E_dPp, P) + torch.einsum('goij,ghij->oh', A_dPp, E_P) \
        + n * u * torch.einsum('goij,ghij->oh', A_dPp, P)
    b["dbw"] = E_dPp.sum((0, 2, 3)) + n * u * A_dPp.sum((0, 2, 3))
    return b


@lru_cache(maxsize=None)
def window_ref_and_bound(c):
    """-> (reference dict, bound dict) in the layout of window_reference; computed once per case and shared."""
    o = window_operands(c)
    N = c.w * c.w
    r, idx = _window_core(o, ident)
    qs = scaled_bf16(o.q, c.scale)
    qw, kw, vw, dw = (to_windows(t, o.geometry) for t in (qs, o.k, o.v, o.do))
    bias = o.table.double()[idx.view(-1)].view(N, N, c.H).permute(2, 0, 1)
    mask = img_mask(c.Hs, c.Ws, c.w, c.ms).repeat(c.B, 1, 1)
    b = _core_bound(r, qw, kw, vw, dw, c.scale, bias, mask, *_mix_fp64(o), c.H if c.mixed else 0)
    bound = {n: from_windows(b[n], o.geometry) for n in ("out", "dq", "dk", "dv")}
    bound["lse"], bound["delta"] = b["lse"], b["delta"]
    # d table: the (i, j) pairs of a bucket, over all windows — their fp32 errors plus one rounding per term summed
    NU = (2 * c.w - 1) ** 2
    pairs = torch.zeros(NU, dtype=torch.float64).index_add_(0, idx.view(-1), torch.ones(N * N, dtype=torch.float64))
    add = lambda t: torch.zeros(NU, c.H, dtype=torch.float64).index_add_(0, idx.view(-1), t.permute(1, 2, 0).reshape(N * N, c.H))  # noqa: E731
    bound["dT"] = add(b["dbias"]) + (pairs * U32).unsqueeze(1) * add(b["A_dbias"])
    if c.mixed:
        bound.update({n: b[n] for n in ("dWl", "dbl", "dWw", "dbw")})
    ref = window_reference(o)
    return ref, bound


@lru_cache(maxsize=None)
def mini_ref_and_bound(c):
    o = mini_operands(c)
    r = _mini_core(o, ident, bf16)                           # M6 and M7 in, every other rounding out
    qs = scaled_bf16(o.q, c.scale)
    perm = lambda t: t.permute(0, 2, 1, 3)                   # noqa: E731
    zero = torch.zeros(c.H, dtype=torch.float64)
    b = _core_bound(r, perm(qs), perm(o.k), perm(o.v), perm(o.do), c.scale, None, None, o.wl.double().view(c.H, c.H), zero,
                    o.ww.double().view(c.H, c.H), zero, c.H, _rpe_terms(o))
    bound = {n: perm(b[n]) for n in ("out", "dq", "dk", "dv")}
    bound.update({n: b[n] for n in ("lse", "delta", "dWl", "dWw")})
    ref = mini_reference(o)
    if o.rpe is not None:
        bound["dWk"] = b["dWk"]
        centre = _mini_pack(o, r)                            # the exactly known effect of M6 and M7 (module docstring)
        bound = {n: t + (centre[n] - ref[n]).abs() for n, t in bound.items()}
    return ref, bound


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 counts as 0; anything over a zero bound as inf)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0
