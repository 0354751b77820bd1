"""Operands for which the bf16 GEMM kernels must be EXACT, and their fp64 references on the CPU.

Operands are drawn from {-1, 0, 1} x 2^s with one power-of-two scale s per tensor.  Every product and every partial sum is
then a small integer times a power of two: fp32 accumulation is exact in any order, and while the magnitude of a result, in
units of its scale, stays <= 256 (`CAP`) the bf16 output is exact too (bf16 holds every integer up to 2^8).  A kernel's output
must then equal the fp64 reference bit for bit (torch.equal) whatever its tile, split, epilogue schedule or grid: a dropped,
duplicated or misaddressed term cannot hide under a tolerance.  The cap is a CONDITION, not a tolerance: every reference below
asserts it before it returns, and tests/test_gemm_exact_ref_cpu.py asserts it over the whole shared case list with the seeds
the GPU tests use.  A case that breaks the cap is a bad case: change its seed or make an operand sparser (`sparse=True`:
the weight is zero with probability 1/2), never the comparison.

Scales: x = t x 2, W = t x 2^-5, so x . W^T is j / 16 with an integer j; bias = t / 16 and, for the GELU epilogue,
bias_gelu = {-32 .. 32} / 16 — h = j / 16 with |j| <= 256 covers the range where GELU is not saturated and is still exact.
dy = t x 2^-2.  `factor` (the saved gelu'(h) of the x gelu' epilogue) is arbitrary bf16 in (0, 1.13]: an exact accumulator
(an integer <= 256) times an 8-bit mantissa is exact in fp32, so that epilogue rounds once.

Everything outside the active block is NaN: wsup[N:], wsup[:, K:] (and the transposed copy the same way), and the rows behind
the M rows of x, dy and factor.  A tail that reads past K, N or M and relies on multiplying by zero shows up as NaN.

The segment-addressed products read the de-interleaved [q | k | v] copy of an interleaved qkv super weight; their reference is
the row gather of qkv_super.py:72-83 (weight rows i, i + 3, .. of the first 3 x nseg rows for part i; contiguous-prefix bias)
as tests/test_block_gpu.py::test_qkv_segment_addressing_matches_row_gather states it.
"""
from collections import namedtuple
from functools import lru_cache
import math

import torch

CAP = 256.0
SX, SW, SDY = 2.0, 2.0 ** -5, 2.0 ** -2          # per-tensor scales; SX * SW = 1 / 16 is the unit of h
UNIT_FWD, UNIT_DGRAD, UNIT_WGRAD, UNIT_BIAS = SX * SW, SDY * SW, SDY * SX, SDY
PAD_ROWS = 8                                      # NaN rows behind the M rows of x / dy / factor

# M, N, K as in cream_linear_fwd: out (M x N) = x (M x K) . W (N x K)^T.  seg: nseg = kseg of the segment-addressed products
# (N == 3 * seg; the stored parts hold seg + 64 rows).  nvalid: cream_linear_gelu_fwd_pad's Nvalid (0 = N).  xzero: columns of x
# from this index on are zero (fc2 over the padded hidden width reads the zero columns fc1 wrote).  sparse: W zero w.p. 1/2.
Case = namedtuple("Case", "M N K seg nvalid xzero sparse seed", defaults=(0, 0, 0, False, 0))


def case_id(c):
    s = f"M{c.M}-N{c.N}-K{c.K}"
    if c.seg:
        s += f"-seg{c.seg}"
    if c.nvalid:
        s += f"-nvalid{c.nvalid}"
    if c.xzero:
        s += f"-xzero{c.xzero}"
    return s


def _ternary(shape, g, p_zero=1.0 / 3.0):
    u = torch.rand(shape, generator=g, dtype=torch.float64)
    nz = (1.0 - p_zero) / 2.0
    return (u < nz).double() - (u > 1.0 - nz).double()


def _poisoned_rows(t, scale):
    """(buffer, view): the first rows hold t x scale as bf16, PAD_ROWS rows of NaN follow."""
    buf = torch.full((t.shape[0] + PAD_ROWS, t.shape[1]), float("nan"), dtype=torch.bfloat16)
    buf[:t.shape[0]] = (t * scale).bfloat16()
    return buf


class Operands:
    """bf16 tensors on the CPU.  x, dy, factor: (M + PAD_ROWS, .) buffers whose first M rows are the operand.
    wsup (N + 64, ldw) with its transposed copy wt (ldw, N + 64); with c.seg also w3 (3, seg + 64, ldw), wt3 (3, ldw, seg + 64)
    and wseg (N, K): the gathered rows as fp64.  bias, bias_gelu: (N + 64,)."""

    def __init__(self, c, seed):
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * c.M + 31 * c.N + c.K + c.seed)
        M, N, K = c.M, c.N, c.K
        self.case, self.ldw = c, K + 8
        xt = _ternary((M, K), g)
        if c.xzero:
            xt[:, c.xzero:] = 0
        self.x = _poisoned_rows(xt, SX)
        self.dy = _poisoned_rows(_ternary((M, N), g), SDY)
        f = (torch.rand((M, K), generator=g) * 1.13).clamp_min(2.0 ** -20).bfloat16().double().clamp_max(1.125)   # (0, 1.13] in bf16
        self.factor = _poisoned_rows(f, 1.0)
        self.bias = torch.full((N + 64,), float("nan"), dtype=torch.bfloat16)
        self.bias[:N] = (_ternary((N,), g) * UNIT_FWD).bfloat16()
        self.bias_gelu = torch.full((N + 64,), float("nan"), dtype=torch.bfloat16)
        self.bias_gelu[:N] = (torch.randint(-32, 33, (N,), generator=g).double() * UNIT_FWD).bfloat16()
        wt_ = _ternary((N, K), g, 0.5 if c.sparse else 1.0 / 3.0)
        self.wsup = torch.full((N + 64, self.ldw), float("nan"), dtype=torch.bfloat16)
        self.wsup[:N, :K] = (wt_ * SW).bfloat16()
        self.wt = self.wsup.t().contiguous()                                     # (ldw, N + 64), poisoned the same way
        if c.seg:
            assert N == 3 * c.seg and c.seg % 64 == 0
            rows = c.seg + 64
            inter = _ternary((3 * rows, K), g, 0.5 if c.sparse else 1.0 / 3.0) * SW       # the interleaved super weight
            self.wseg = torch.cat([inter[i:3 * c.seg:3] for i in range(3)], 0)   # the reference's row gather
            self.w3 = torch.full((3, rows, self.ldw), float("nan"), dtype=torch.bfloat16)
            for i in range(3):
                self.w3[i, :c.seg, :K] = inter[i::3][:c.seg].bfloat16()
            self.wt3 = self.w3.transpose(1, 2).contiguous()                      # (3, ldw, rows)

    # -- exact fp64 views of the active blocks
    @property
    def X(self):
        return self.x[:self.case.M].double()

    @property
    def DY(self):
        return self.dy[:self.case.M].double()

    @property
    def F(self):
        return self.factor[:self.case.M].double()

    @property
    def W(self):
        return self.wsup[:self.case.N, :self.case.K].double()


@lru_cache(maxsize=4)
def operands(case, seed=0):
    return Operands(case, seed)


def _exact(v, unit, what):
    """The exactness cap, then the bf16 value (the rounding is the identity under the cap)."""
    peak = float(v.abs().max()) / unit if v.numel() else 0.0
    assert peak <= CAP, f"{what}: |value| reaches {peak} units of {unit} > {CAP}: bad case (change the seed or make an operand sparser)"
    assert torch.equal(v / unit, (v / unit).round()), f"{what}: not a multiple of its unit"
    out = v.bfloat16()
    assert torch.equal(out.double(), v), f"{what}: not representable in bf16"
    return out


def ref_fwd(o, bias=True):
    v = o.X @ o.W.t()
    if bias:
        v = v + o.bias[:o.case.N].double()
    return _exact(v, UNIT_FWD, "forward" + (" + bias" if bias else ""))


def ref_fwd_seg(o, bias=True):
    v = o.X @ o.wseg.t()
    if bias:
        v = v + o.bias[:o.case.N].double()
    return _exact(v, UNIT_FWD, "segment-addressed forward")


def ref_dgrad(o):
    return _exact(o.DY @ o.W, UNIT_DGRAD, "dgrad")


def ref_dgrad_seg(o):
    return _exact(o.DY @ o.wseg, UNIT_DGRAD, "segment-addressed dgrad")


def ref_dgrad_mul(o):
    """-> (bf16((dy . W) x factor), the fp64 product before the rounding): one rounding, see the module docstring."""
    acc = _exact(o.DY @ o.W, UNIT_DGRAD, "dgrad before x factor").double()
    prod = acc * o.F                                  # <= 9 bits x 8 bits: exact in fp32 and fp64
    assert torch.equal(prod.float().double(), prod)
    return prod.float().bfloat16(), prod


def gelu64(h):
    return h * 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))


def gelu_grad64(h):
    return 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def ref_gelu(o):
    """-> (h bf16 exact, gelu(h) fp64, gelu'(h) fp64); columns >= nvalid are zero in both outputs."""
    c = o.case
    h = _exact(o.X @ o.W.t() + o.bias_gelu[:c.N].double(), UNIT_FWD, "h of the GELU epilogue")
    hd = h.double()
    g, gp = gelu64(hd), gelu_grad64(hd)
    if c.nvalid:
        g[:, c.nvalid:] = 0
        gp[:, c.nvalid:] = 0
    return h, g, gp


def gelu_bound(ref, h):
    """One bf16 ulp of the value plus twice the |err| <= 5e-7 of the kernels' A&S 7.1.26 erf (scaled by |h| where it is multiplied in)."""
    return 2.0 ** -8 * ref.abs() + 1e-6 * h.abs().clamp_min(1.0)


def wgrad_slices(M, S):
    """Token slices of the split-K weight gradients: whole 64-row steps, as even as possible."""
    steps = (M + 63) // 64
    return [(steps * s // S * 64, min(M, steps * (s + 1) // S * 64)) for s in range(S)]


def ref_wgrad(o):
    """dy^T x over all tokens, fp64 (the fp32 partials add up to it exactly)."""
    v = o.DY.t() @ o.X
    _exact(v, UNIT_WGRAD, "weight gradient")
    return v


def ref_wgrad_parts(o, S):
    """(S, N, K) bf16: the exact product over each token slice."""
    return torch.stack([_exact(o.DY[lo:hi].t() @ o.X[lo:hi], UNIT_WGRAD, f"weight-gradient slice {lo}:{hi}")
                        for lo, hi in wgrad_slices(o.case.M, S)])


def wgrad_cap_for_every_split(o):
    """max over elements of (largest - smallest prefix sum over whole 64-row steps) in units: bounds |dy_s^T x_s| of EVERY slice
    of whole steps, i.e. for every split count a device may choose."""
    c = o.case
    run = torch.zeros(c.N, c.K, dtype=torch.float64)
    hi, lo = run.clone(), run.clone()
    for r in range(0, c.M, 64):
        run = run + o.DY[r:r + 64].t() @ o.X[r:r + 64]
        hi, lo = torch.maximum(hi, run), torch.minimum(lo, run)
    return float((hi - lo).max()) / UNIT_WGRAD


def ref_colsum_dy(o):
    v = o.DY.sum(0)
    assert float(v.abs().max()) / UNIT_BIAS < 2.0 ** 24
    return v


# ---- the shared case list ------------------------------------------------------------------------------------------------------
TAILS = [64 * 2 + r for r in (8, 16, 24, 32, 40, 48, 56)] + [8, 24, 56, 64, 72, 120, 128]     # K = 64 q + r (q = 2) and zero / one / two K-steps
TAILS_LONG = [1152 + r for r in (0, 8, 16, 24, 32, 40, 48, 56)]                               # the 256 x 256 two-stage tile in its default mode
ROWS = [1, 8, 127, 129, 600, 1032]

# NT kernel families: name -> (switches, W = output width of the sweep, M of the sweep, contractions, ntopt values)
NT_FAMILIES = {
    "128x64": (dict(nt8=0, nt256=0, nthalf=0), 104, 264, TAILS, (0, 3, 11)),
    "128x128": (dict(nt8=0, nt256=0, nthalf=0), 648, 264, TAILS, (0, 3, 11)),
    "256x256-wide": (dict(nt8=0, nt256=1, nthalf=0), 968, 264, TAILS, (3,)),
    "256x256-longK": (dict(nt8=0, nt256=2, nthalf=0), 264, 264, TAILS_LONG, (3,)),
    "nt8": (dict(nt8=1, nthalf=0), 264, 264, TAILS, (3,)),
    "default": (dict(), 256, 264, TAILS, (3,)),           # cream_linear_fwd(N = 256) -> gemm_nt8 under the default mode 4
    "256x192-N320": (dict(nt8=0, nt256=0, nthalf=1), 320, 1032, TAILS, (3,)),
    "256x192-N384": (dict(nt8=0, nt256=0, nthalf=1), 384, 1032, TAILS, (3,)),
}


def sweep_pair(W, M, c):
    """A contraction length c under an output W wide: the forward-type products contract over K, the dgrad-type ones over N."""
    return Case(M, W, c), Case(M, c, W)


def _row_contraction(fam):
    return 1160 if fam == "256x256-longK" else 200


TAIL_CASES = [(fam, c) for fam, (_, W, M, cs, _) in NT_FAMILIES.items() for c in cs]
# (the 256 x 192 tile serves M >= 1024 only: its row edges are 1 and 8 rows into the fifth row tile)
ROW_CASES = [(fam, M) for fam in NT_FAMILIES for M in ((1025, 1032) if fam.startswith("256x192") else ROWS)]

TN_SHAPES = [(200, 264), (528, 624), (624, 200), (264, 528)]
TN_ROWS = [8, 56, 64, 72, 264, 600]
TN_CASES = [Case(M, N, K) for (N, K) in TN_SHAPES for M in TN_ROWS]

# search-space shapes at M = 600: (E, Q = 64 H, F = hidden width; 760 = 756 padded)
MS = 600


def _space(E, Qs, Fs):
    out = []
    for Q in Qs:
        out += [Case(MS, 3 * Q, E, seg=Q), Case(MS, E, Q)]                        # qkv (segment addressing), proj
    for F in Fs:
        if F == 760:
            out += [Case(MS, 760, E, nvalid=756), Case(MS, E, 760, xzero=756)]     # fc1 + GELU padded, fc2 over the zero columns
        else:
            out += [Case(MS, F, E), Case(MS, E, F)]                                # fc1 + GELU, fc2 (and its x gelu' dgrad)
    return out


SPACE_T = _space(192, (192, 256), (672, 768)) + _space(216, (192, 256), (760, 864)) + _space(240, (192, 256), (840, 960))
SPACE_B = (_space(528, (512, 576), (1584, 1848, 2112)) + _space(576, (576, 640), (1728, 2016, 2304)) +
           _space(624, (512, 640), (1872, 2184, 2496)))
SPACE_CASES = SPACE_T + SPACE_B

# small grids: (family, forward-type case, dgrad-type case).  Tiles at M = 1032 against the workgroups 8 CUs hold:
#   128 x 64 x3/CU: 9 x 9 = 81 tiles / 24;  128 x 128 x2/CU: 9 x 6 = 54 / 16;  256 x 256 (both kernels): 5 x 6 = 30 / 8;
#   256 x 192: 5 x 2 = 10 / 8 (N is 320 or 384 and M <= 1032: the most this family can have here)
GRID_CASES = [
    ("128x64", Case(1032, 520, 200), Case(1032, 200, 520)),
    ("128x128", Case(1032, 648, 200), Case(1032, 200, 648)),
    ("256x256-wide", Case(1032, 1288, 200), Case(1032, 200, 1288)),
    ("nt8", Case(1032, 1288, 200), Case(1032, 200, 1288)),
    ("256x192-N384", Case(1032, 384, 200), Case(1032, 200, 384)),
]
GRID_TN_CASE = Case(600, 528, 264)                     # 3 x 2 macro tiles: token slices for half the CUs -> S follows the budget


def all_cases():
    """Every Case of every list above, once."""
    seen, out = set(), []
    for fam, c in TAIL_CASES:
        _, W, M, _, _ = NT_FAMILIES[fam]
        for case in sweep_pair(W, M, c):
            out.append(case)
    for fam, M in ROW_CASES:
        out += list(sweep_pair(NT_FAMILIES[fam][1], M, _row_contraction(fam)))
    out += TN_CASES + SPACE_CASES + [GRID_TN_CASE]
    for _, a, b in GRID_CASES:
        out += [a, b]
    uniq = []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq
