"""fp64 reference, rounding model, per-element bounds and the shared case list for the kernel-level tests of
csrc/token_dwconv.hip (depthwise 3 x 3 convolution on the token layout).

The reference is the operation as the MODEL states it (TinyViT/models/tiny_vit.py:374-376): a literal transpose of the
(B, L, C) token stream to NCHW, `F.conv2d(groups=C, padding=1)` in fp64, the transpose back, and fp64 autograd for every
gradient.  Nothing in it follows the kernels' index arithmetic.

`kernel_model` is the same arithmetic written out by hand as shifted slices, in fp32 and in the kernels' order, with a bf16
rounding where the kernels have one — and with the injected faults the bound must catch.

Rounding points of token_dwconv.hip (u = 2^-24; the build has -ffp-contract=off, so a product and its addition round
separately):
    y      = bias + sum_k w_k x_k     9 fp32 products, 9 additions in a chain that starts at the bias (without a bias the first
                                      addition is exact).  A term is rounded once as a product and once per addition it passes
                                      through, at most 9:                        E(y)  = 10 u A(y)
    dx     = sum_k w_k dy_k           9 products, 8 additions:                    E(dx) =  9 u A(dx)
    dw_k   = sum_n dy_n x_n           n <= B L products; a thread's chain over its tokens, the workgroup's slots through LDS,
                                      the caller's sum of the partials: one rounding per term per addition, whatever the
                                      order — a term passes through at most n - 1 inexact additions (adding an exact zero
                                      rounds nothing):                            E(dw) = n u A(dw)
    dbias  = sum_n dy_n               no products:                                E(db) = (n - 1) u A(db)
    A(.) is the formula with every factor replaced by its absolute value.  First order.  bf16 I/O adds half a bf16 ulp at
    |ref| + E for the store of y and dx; fp32 I/O stores the accumulator itself.  dw and dbias never pass through bf16.
No constant is fitted.
"""
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

from attn_mix_ref import SEED, U32, hu, worst_ratio  # noqa: F401  (worst_ratio: for the tests)

CCase = namedtuple("CCase", "group B Hs Ws C")

FAULTS = ("taps_transposed", "row_end_read_through", "image_read_through", "dx_taps_unflipped", "last_vector_copied")
OUTPUTS = ("y", "dx", "dw", "db")


def _cases():
    cs = []
    # every map with two widths, every width with several maps; B = 1 and 3 alternate
    grid = [((1, 1), (8, 576)), ((1, 4), (40, 160)), ((3, 1), (64, 8)), ((2, 2), (160, 40)), ((3, 3), (576, 64)),
            ((5, 9), (40, 576)), ((7, 7), (64, 160)), ((14, 14), (8, 576))]
    for n, ((Hs, Ws), widths) in enumerate(grid):
        for m, C in enumerate(widths):
            cs.append(CCase("map", 1 if (n + m) % 2 == 0 else 3, Hs, Ws, C))
    return cs


CASES = _cases()
# more tokens than one pass of either grid at C = 576 (3 token slots per workgroup in bf16, 1 in fp32): the workgroups loop
MANY_CASES = [CCase("many", 3, 48, 48, 576), CCase("many", 2, 300, 301, 8)]


def cid(c):
    return f"{c.group}-{c.Hs}x{c.Ws}-C{c.C}-B{c.B}"


class Operands:
    """x, dy (B, L, C) bf16-representable fp32; w (C, 1, 3, 3) and bias (C) fp32, asymmetric taps."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(SEED + 2750159 + 104729 * (CASES + MANY_CASES).index(c))
        L = c.Hs * c.Ws
        self.case = c
        self.x = torch.randn(c.B, L, c.C, generator=g).bfloat16().float()
        self.dy = torch.randn(c.B, L, c.C, generator=g).bfloat16().float()
        self.w = 0.5 * torch.randn(c.C, 1, 3, 3, generator=g) + 0.1 * torch.arange(9.0).view(1, 1, 3, 3)      # no symmetry
        self.bias = 0.5 * torch.randn(c.C, generator=g)


@lru_cache(maxsize=None)
def operands(c):
    return Operands(c)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _nchw(t, c):
    return t.transpose(1, 2).reshape(c.B, c.C, c.Hs, c.Ws)


def _tokens(t, c):
    return t.reshape(c.B, c.C, c.Hs * c.Ws).transpose(1, 2)


def reference(o, bias):
    """-> {y, dx, dw, db} fp64 (db None without a bias... it is computed anyway: the kernels always return it)."""
    c = o.case
    x = o.x.double().requires_grad_(True)
    w = o.w.double().requires_grad_(True)
    b = o.bias.double().requires_grad_(True)
    y = _tokens(F.conv2d(_nchw(x, c), w, b if bias else None, padding=1, groups=c.C), c)
    if not bias:
        y = y + 0.0 * b.view(1, 1, -1)
    dx, dw, _ = torch.autograd.grad(y, (x, w, b), o.dy.double())
    return dict(y=y.detach(), dx=dx, dw=dw, db=o.dy.double().sum((0, 1)))


def _absolute(o, bias):
    """A(.) of every output: the formulas with every factor replaced by its absolute value."""
    c = o.case
    ax, ady, aw = o.x.double().abs(), o.dy.double().abs(), o.w.double().abs()
    ab = o.bias.double().abs() if bias else torch.zeros(c.C, dtype=torch.float64)
    Ay = _tokens(F.conv2d(_nchw(ax, c), aw, ab, padding=1, groups=c.C), c)
    Adx = _tokens(F.conv_transpose2d(_nchw(ady, c), aw, padding=1, groups=c.C), c)
    xp = F.pad(_nchw(ax, c), (1, 1, 1, 1))
    g = _nchw(ady, c)
    Adw = torch.stack([torch.stack([(g * xp[:, :, di:di + c.Hs, dj:dj + c.Ws]).sum((0, 2, 3)) for dj in range(3)], -1)
                       for di in range(3)], -2).view(c.C, 1, 3, 3)
    return dict(y=Ay, dx=Adx, dw=Adw, db=ady.sum((0, 1)))


@lru_cache(maxsize=None)
def ref_and_bound(c, bf16_io, bias):
    """-> (reference dict, bound dict), computed once per (case, I/O type, bias) and shared."""
    o = operands(c)
    r, A = reference(o, bias), _absolute(o, bias)
    n = c.B * c.Hs * c.Ws
    E = dict(y=10 * U32 * A["y"], dx=9 * U32 * A["dx"], dw=n * U32 * A["dw"], db=(n - 1) * U32 * A["db"])
    if bf16_io:
        for k in ("y", "dx"):
            E[k] = E[k] + hu(r[k].abs() + E[k])
    return r, E


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
    if fault == "row_end_read_through":                     # no zero padding in j: the neighbouring row's end token is read
        ok = row_ok & (src >= 0) & (src < B * L) & (src // L == tok // L)
    elif fault == "image_read_through":                     # no zero padding in i between images: image b - 1's last row is read
        ok = col_ok & (src >= 0) & (src < B * L)
    else:
        ok = row_ok & col_ok
    flat = t.reshape(B * L, -1)
    return torch.where(ok.view(-1, 1), flat[src.clamp(0, B * L - 1)], torch.zeros((), dtype=t.dtype)).view(B, L, -1)


def _store(t, bf16_io):
    return t.bfloat16().float() if bf16_io else t


def kernel_model(o, bf16_io, bias, fault=None):
    """-> {y, dx, dw, db} as the kernels compute them: fp32, bias first, taps in row-major order, products and additions
    separate, one bf16 rounding on the store of y and dx."""
    c = o.case
    w = o.w.view(c.C, 3, 3)
    wf = w.transpose(1, 2) if fault == "taps_transposed" else w
    y = (o.bias if bias else torch.zeros(c.C)).view(1, 1, -1).expand(c.B, c.Hs * c.Ws, c.C).clone()
    dx = torch.zeros_like(y)
    dw = torch.zeros(c.C, 3, 3)
    for di in range(3):
        for dj in range(3):
            xs = _shifted(o.x, c, di - 1, dj - 1, fault)
            y = y + wf[:, di, dj].view(1, 1, -1) * xs
            tap = wf[:, di, dj] if fault == "dx_taps_unflipped" else wf[:, 2 - di, 2 - dj]
            dx = dx + tap.view(1, 1, -1) * _shifted(o.dy, c, di - 1, dj - 1, fault)
            dw[:, di, dj] = (o.dy * xs).sum((0, 1))
    if fault == "taps_transposed":
        dw = dw.transpose(1, 2)
    y, dx = _store(y, bf16_io), _store(dx, bf16_io)
    if fault == "last_vector_copied" and c.C >= 16:
        y, dx = y.clone(), dx.clone()
        y[..., -8:], dx[..., -8:] = y[..., -16:-8], dx[..., -16:-8]
        dw = dw.clone()
        dw[-8:] = dw[-16:-8]
    return dict(y=y, dx=dx, dw=dw.view(c.C, 1, 3, 3), db=o.dy.sum((0, 1)))
