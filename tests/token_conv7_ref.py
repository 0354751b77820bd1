"""fp64 reference, rounding model, per-element bounds and the shared case list for the kernel-level tests of
csrc/token_dwconv7.hip (depthwise 7 x 7 convolution on the token layout, residual r in {0, 1} fused).

The reference is the operation as the MODEL states it (MiniViT/Mini-Swin/models/swin_transformer_minivit.py:328-332): a literal
transpose of the (B, L, C) token stream to NCHW, `F.conv2d(groups=C, padding=3)` in fp64, the residual, the transpose back, and
fp64 autograd for every gradient.  Nothing in it follows the kernels' index arithmetic.

`kernel_model` is the same arithmetic written out by hand as shifted token gathers, in fp32 and in the kernels' order, with a
bf16 rounding where the kernels have one — and with the injected faults the bound must catch.

Rounding points of token_dwconv7.hip (u = 2^-24; the build has -ffp-contract=off, so a product and its addition round
separately).  The summation order does not matter: a term is rounded once as a product and once per addition it passes through.
    y      = bias + sum_k w_k x_k (+ x)   49 products, 49 additions in a chain that starts at the bias, r for the residual: a
                                          term passes through at most 49 + r additions:     E(y)  = (50 + r) u A(y)
    dx     = sum_k w_k dy_k (+ dy)        49 products, 48 additions, r for the residual:     E(dx) = (49 + r) u A(dx)
    dw_k   = sum_n dy_n x_n               n = B Hs Ws products; a thread's chain over its strips, the workgroup's 8 groups
                                          through LDS, the caller's sum of the partials: at most n - 1 inexact additions per
                                          term (adding an exact zero rounds nothing):        E(dw) = n u A(dw)
    dbias  = sum_n dy_n                   no products:                                       E(db) = (n - 1) u A(db)
    A(.) is the formula with every factor replaced by its absolute value.  First order.  bf16 I/O adds half a bf16 ulp at
    |ref| + E for the store of y and dx; fp32 I/O stores the accumulator itself.  dw and dbias never pass through bf16.
No constant is fitted.

The kernels' tile is 14 x 14 tokens x 32 channels (strips of 7 outputs); the case list is built around those edges.
"""
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

from attn_mix_ref import SEED, U32, hu, worst_ratio  # noqa: F401  (worst_ratio: for the tests)

CCase = namedtuple("CCase", "group B Hs Ws C")

TILE, CHUNK = 14, 32                                    # csrc/token_dwconv7.hip: TILE, CCH
FAULTS = ("taps_transposed", "row_end_read_through", "image_read_through", "dx_taps_unflipped", "last_vector_copied",
          "y_residual_dropped", "dx_residual_dropped", "outer_ring_ignored", "halo_off_by_one")
OUTPUTS = ("y", "dx", "dw", "db")


def _cases():
    cs = []
    # every map with two widths; B = 1 and 3 alternate.  1x1 .. 3x3: every tap row partly outside; 4x7, 7x7, 6x8: a strip of 7
    # exactly covers the row, or just fails to; 5x9, 15x9, 9x17: Hs != Ws; 13, 14, 15 in each axis: the tile's edge - 1, the
    # edge, the edge + 1.  C: 8 below, 32 at, 40 above the channel chunk (40: the last chunk has 8 of 32 lanes busy).
    grid = [((1, 1), (8, 1024)), ((1, 4), (40, 160)), ((3, 1), (96, 8)), ((2, 2), (160, 32)), ((3, 3), (576, 128)),
            ((4, 7), (40, 96)), ((7, 7), (128, 1024)), ((6, 8), (8, 160)), ((5, 9), (32, 576)), ((15, 9), (40, 96)),
            ((9, 17), (160, 8)), ((14, 14), (8, 576)), ((13, 15), (40, 128)), ((15, 13), (96, 32))]
    for n, ((Hs, Ws), widths) in enumerate(grid):
        for m, C in enumerate(widths):
            cs.append(CCase("map", 1 if (n + m) % 2 == 0 else 3, Hs, Ws, C))
    return cs


CASES = _cases()
R0_CASES = [c for c in CASES if (c.Hs, c.Ws) in ((1, 1), (2, 2), (7, 7), (9, 17), (14, 14), (15, 13))]      # r = 0 as well
# more tiles than the grid has workgroups along the tile axis: the workgroups of every launch loop
# (5 x 4 = 20 tiles on 2 x 256 / 32 = 16 workgroups per channel chunk, 968 tiles on 512); the first has edge tiles one token wide
MANY_CASES = [CCase("many", 5, 15, 15, 1024), CCase("many", 2, 300, 301, 8)]


def cid(c):
    return f"{c.group}-{c.Hs}x{c.Ws}-C{c.C}-B{c.B}"


def tiles(c):
    return c.B * -(-c.Hs // TILE) * -(-c.Ws // TILE)


class Operands:
    """x, dy (B, L, C) bf16-representable fp32; w (C, 1, 7, 7) and bias (C) fp32, asymmetric taps."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(SEED + 15485863 + 104729 * (CASES + MANY_CASES).index(c))
        L = c.Hs * c.Ws
        self.case = c
        self.x = torch.randn(c.B, L, c.C, generator=g).bfloat16().float()
        self.dy = torch.randn(c.B, L, c.C, generator=g).bfloat16().float()
        self.w = 0.25 * torch.randn(c.C, 1, 7, 7, generator=g) + 0.02 * torch.arange(49.0).view(1, 1, 7, 7)      # no symmetry
        self.bias = 0.5 * torch.randn(c.C, generator=g)


@lru_cache(maxsize=None)
def operands(c):
    return Operands(c)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _nchw(t, c):
    return t.transpose(1, 2).reshape(c.B, c.C, c.Hs, c.Ws)


def _tokens(t, c):
    return t.reshape(c.B, c.C, c.Hs * c.Ws).transpose(1, 2)


def reference(o, bias, r):
    """-> {y, dx, dw, db} fp64 (db is computed with or without a bias: the kernels always return it)."""
    c = o.case
    x = o.x.double().requires_grad_(True)
    w = o.w.double().requires_grad_(True)
    b = o.bias.double()
    xm = _nchw(x, c)
    ym = F.conv2d(xm, w, b if bias else None, padding=3, groups=c.C)
    if r:
        ym = xm + ym
    y = _tokens(ym, c)
    dx, dw = torch.autograd.grad(y, (x, w), o.dy.double())
    return dict(y=y.detach(), dx=dx, dw=dw, db=o.dy.double().sum((0, 1)))


def _absolute(o, bias, r):
    """A(.) of every output: the formulas with every factor replaced by its absolute value."""
    c = o.case
    ax, ady, aw = o.x.double().abs(), o.dy.double().abs(), o.w.double().abs()
    ab = o.bias.double().abs() if bias else torch.zeros(c.C, dtype=torch.float64)
    Ay = _tokens(F.conv2d(_nchw(ax, c), aw, ab, padding=3, groups=c.C), c) + r * ax
    Adx = _tokens(F.conv_transpose2d(_nchw(ady, c), aw, padding=3, groups=c.C), c) + r * ady
    xp = F.pad(_nchw(ax, c), (3, 3, 3, 3))
    g = _nchw(ady, c)
    Adw = torch.stack([torch.stack([(g * xp[:, :, di:di + c.Hs, dj:dj + c.Ws]).sum((0, 2, 3)) for dj in range(7)], -1)
                       for di in range(7)], -2).view(c.C, 1, 7, 7)
    return dict(y=Ay, dx=Adx, dw=Adw, db=ady.sum((0, 1)))


@lru_cache(maxsize=None)
def ref_and_bound(c, bf16_io, bias, r=1):
    """-> (reference dict, bound dict), computed once per (case, I/O type, bias, residual) and shared."""
    o = operands(c)
    ref, A = reference(o, bias, r), _absolute(o, bias, r)
    n = c.B * c.Hs * c.Ws
    E = dict(y=(50 + r) * U32 * A["y"], dx=(49 + r) * U32 * A["dx"], dw=n * U32 * A["dw"], db=(n - 1) * U32 * A["db"])
    if bf16_io:
        for k in ("y", "dx"):
            E[k] = E[k] + hu(ref[k].abs() + E[k])
    return ref, E


# ---- the kernels' arithmetic by hand, with the injected faults ------------------------------------------------------------------
def _shifted(t, c, oi, oj, fault=None):
    """t (B, L, C) -> s with s[b, i, j] = t[b, i + oi, j + oj] inside the map and 0 outside, as flat token arithmetic."""
    B, L = c.B, c.Hs * c.Ws
    tok = torch.arange(B * L)
    n = tok % L
    i, j = n // c.Ws, n % c.Ws
    row_ok = (i + oi >= 0) & (i + oi < c.Hs)
    col_ok = (j + oj >= 0) & (j + oj < c.Ws)
    src = tok + oi * c.Ws + oj
    if fault == "row_end_read_through":                     # no zero padding in j: the neighbouring row's end tokens are read
        ok = row_ok & (src >= 0) & (src < B * L) & (src // L == tok // L)
    elif fault == "image_read_through":                     # no zero padding in i: the token arithmetic runs on into the
        ok, src = col_ok, src % (B * L)                     # neighbouring image (around the ends of the buffer)
    else:
        ok = row_ok & col_ok
    flat = t.reshape(B * L, -1)
    return torch.where(ok.view(-1, 1), flat[src.clamp(0, B * L - 1)], torch.zeros((), dtype=t.dtype)).view(B, L, -1)


def _store(t, bf16_io):
    return t.bfloat16().float() if bf16_io else t


def kernel_model(o, bf16_io, bias, r=1, fault=None):
    """-> {y, dx, dw, db} as the kernels compute them: fp32, bias first, the 49 products in row-major order of the input offset,
    products and additions separate, the residual last, one bf16 rounding on the store of y and dx.

    Faults: taps_transposed (w[c, dj, di]); row_end_read_through / image_read_through (see _shifted); dx_taps_unflipped;
    last_vector_copied (the last 4-channel staging vector repeats the one before it); y_residual_dropped / dx_residual_dropped;
    outer_ring_ignored (a 5 x 5 stencil: the taps at distance 3 skipped); halo_off_by_one (the staged tile starts one token
    late in both axes: every read of the stencil, the residual's included, lands at (+1, +1))."""
    c = o.case
    w = o.w.view(c.C, 7, 7)
    wf = w.transpose(1, 2) if fault == "taps_transposed" else w
    off = 1 if fault == "halo_off_by_one" else 0
    y = (o.bias if bias else torch.zeros(c.C)).view(1, 1, -1).expand(c.B, c.Hs * c.Ws, c.C).clone()
    dx = torch.zeros_like(y)
    dw = torch.zeros(c.C, 7, 7)
    for di in range(7):
        for dj in range(7):
            ring = fault == "outer_ring_ignored" and max(abs(di - 3), abs(dj - 3)) == 3
            xs = _shifted(o.x, c, di - 3 + off, dj - 3 + off, fault)
            if not ring:
                y = y + wf[:, di, dj].view(1, 1, -1) * xs
                tap = wf[:, di, dj] if fault == "dx_taps_unflipped" else wf[:, 6 - di, 6 - dj]
                dx = dx + tap.view(1, 1, -1) * _shifted(o.dy, c, di - 3 + off, dj - 3 + off, fault)
                dw[:, di, dj] = (o.dy * xs).sum((0, 1))
    if fault == "taps_transposed":
        dw = dw.transpose(1, 2)
    if r and fault != "y_residual_dropped":
        y = y + _shifted(o.x, c, off, off)
    if r and fault != "dx_residual_dropped":
        dx = dx + _shifted(o.dy, c, off, off)
    y, dx = _store(y, bf16_io), _store(dx, bf16_io)
    if fault == "last_vector_copied":
        y, dx = y.clone(), dx.clone()
        y[..., -4:], dx[..., -4:] = y[..., -8:-4], dx[..., -8:-4]
        dw = dw.clone()
        dw[-4:] = dw[-8:-4]
    return dict(y=y, dx=dx, dw=dw.reshape(c.C, 1, 7, 7), db=o.dy.sum((0, 1)))
