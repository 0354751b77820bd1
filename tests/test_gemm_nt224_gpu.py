"""The 256 x 224 NT tile on 16x16x32 MFMAs (csrc/gemm_nt224.hpp; launch_nt224, cream_gemm_nt224 and cream_linear_nt224 in
csrc/gemm_mfma.hip).

Exact operands (tests/gemm_exact_ref.py: ternary x a power of two) must come out bit for bit equal to the fp64 CPU reference:
bias, no bias and the plain store (the dgrad orientation: contraction over the reference's N) for
  * every contraction K in 8 / 24 / 56 / 64 / 72 / 120 / 128 / 448 / 1160 / 1344 (zero, one, two K-steps with and without a
    tail, long ones) at N = 448 (two whole column tiles) and 456 (a third tile that sticks out by 8 columns), M = 257;
  * every N in 224 / 448 / 456 / 672 / 1344 against every M in 1 / 8 / 127 / 129 / 255 / 257 / 600 / 1032 at K = 72;
  * segment addressing at M = 1032: forward nseg = 448 at N = 1344, dgrad kseg = 320 / 448 at N = 448 — through
    cream_linear_nt224 and through cream_linear_fwd_seg / cream_linear_dgrad_seg, which the switch routes to the tile;
  * persistent grids smaller than the problem (30 tiles on 8 and 24 CUs): the same bits at every CU budget.
cream_linear_nt224 runs the tile on any shape; launch_nt routes N == 448 (and the qkv forward N == 1344 in
segments of 448) at M >= 1024 to it while cream_gemm_nt224 is on: the
routed calls must give the tile's bits.  Every output sits in front of a guard band; the switch and the CU budget are restored.

Random bf16 operands at (M, N, K) = (1032, 448, 448) and (1032, 448, 1344): every element within 2^-8 |c| (one bf16 rounding of
the result) + K 2^-24 sum |a| |b| (fp32 accumulation of K terms in any order) of the fp64 product c of the bf16 operands; reruns
bit-identical.  The switch-off kernels add 16 contraction elements per MFMA, this tile 32: both roundings of nearby fp32 sums
land on the same or on neighbouring bf16 values: the same call with the switch off must agree within one bf16 ulp element-wise.
That is asserted on these signed operands and again on their absolute values (c >= sum |a| |b|: no result is the remainder of a
cancellation, so the fp32 sums provably differ by less than a bf16 ulp of the result); the switch-off result is held to the
fp64 bound too.

Routing: cream_gemm_nt224_launches counts the tile's launches, so the routed calls above must add one and the calls outside the
rule (switch off, M < 1024, other widths, N = 1344 in one segment) none."""
import contextlib
import ctypes

import pytest
import torch

import gemm_exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16

KS = [8, 24, 56, 64, 72, 120, 128, 448, 1152 + 8, 1344]
NS = [224, 448, 456, 672, 1344]
MS = [1, 8, 127, 129, 255, 257, 600, 1032]


def _lib():
    from cream_amd import _lib as L
    return L.load()


def _check(rc, what):
    from cream_amd import _lib as L
    L.check(rc, what)


@contextlib.contextmanager
def switch(name, value):
    fn = getattr(_lib(), name)
    was = fn(value)
    try:
        yield
    finally:
        fn(was)


@pytest.fixture(scope="module", autouse=True)
def _switches_untouched():
    lib = _lib()
    before = (lib.cream_gemm_nt224(-1), lib.cream_cu_reserve(-1))
    yield
    after = (lib.cream_gemm_nt224(-1), lib.cream_cu_reserve(-1))
    lib.cream_gemm_nt224(before[0])
    lib.cream_cu_reserve(before[1])
    assert after == before


class Guard:
    """Outputs as views into buffers filled with -7 with a guard band behind them."""

    def __init__(self):
        self.bufs = []

    def new(self, *shape):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 4096,), -7.0, device=DEV, dtype=BF16)
        self.bufs.append((buf, n))
        return buf[:n].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool((buf[n:] == -7).all()), "the kernel wrote behind its output"


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nt224(out, a, b, bias, M, N, K, ldb, nseg=0, nseg_stride=0, kseg=0, kseg_stride=0):
    """out (M x N) = a (M x K) . b (N x K)^T (+ bias) on the 256 x 224 tile, whatever the shape."""
    _check(_lib().cream_linear_nt224(_p(out), _p(a), _p(b), _p(bias), M, N, K, ldb, nseg, nseg_stride, kseg, kseg_stride,
                                     _stream()), "cream_linear_nt224")
    return out


@contextlib.contextmanager
def tile_launches(n):
    """The calls inside launch the 256 x 224 tile exactly n times (cream_gemm_nt224_launches counts them)."""
    lib = _lib()
    before = lib.cream_gemm_nt224_launches()
    yield
    got = lib.cream_gemm_nt224_launches() - before
    assert got == n, f"{got} launches of the 256 x 224 tile, expected {n}"


def _finite(name, t):
    assert bool(torch.isfinite(t).all()), f"{name}: NaN / inf — a read past K, N or M (the poison) or a lost store"


def run_exact(fwd_case, bwd_case):
    """Bias, no bias (contracting over K of fwd_case) and the plain store (contracting over N of bwd_case) — twice."""
    of, ob = R.operands(fwd_case, 0), R.operands(bwd_case, 0)
    c, b = fwd_case, bwd_case
    x, w, bias = of.x.to(DEV)[:c.M], of.wsup.to(DEV), of.bias.to(DEV)
    dy, wt = ob.dy.to(DEV)[:b.M], ob.wt.to(DEV)
    want = dict(out=R.ref_fwd(of), out0=R.ref_fwd(of, False), dx=R.ref_dgrad(ob))
    runs = []
    for _ in range(2):
        G = Guard()
        res = dict(out=nt224(G.new(c.M, c.N), x, w, bias, c.M, c.N, c.K, w.stride(0)),
                   out0=nt224(G.new(c.M, c.N), x, w, None, c.M, c.N, c.K, w.stride(0)),
                   dx=nt224(G.new(b.M, b.K), dy, wt, None, b.M, b.K, b.N, wt.stride(0)))
        G.check()
        for k, v in res.items():
            _finite(k, v)
            assert torch.equal(v.cpu(), want[k]), (k, R.case_id(c if k != "dx" else b))
        runs.append(res)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k}: the rerun differs"
    return runs[0]


@pytest.mark.parametrize("N", [448, 456])
@pytest.mark.parametrize("K", KS)
def test_contraction_tails_are_exact(K, N):
    run_exact(R.Case(257, N, K), R.Case(257, K, N))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
def test_row_and_column_edges_are_exact(N, M):
    run_exact(R.Case(M, N, 72), R.Case(M, 72, N))


@pytest.mark.parametrize("M,N,K", [(1032, 1344, 1344), (1032, 448, 1160), (600, 672, 448)])
def test_long_contractions_over_several_tiles_are_exact(M, N, K):
    run_exact(R.Case(M, N, K), R.Case(M, K, N))


def test_forward_row_segments_are_exact():
    """qkv forward at 7 heads: N = 1344 in three row segments of 448 = two whole column tiles each."""
    c = R.Case(1032, 1344, 200, seg=448)
    o = R.operands(c, 0)
    x, w3, bias = o.x.to(DEV)[:c.M], o.w3.to(DEV), o.bias.to(DEV)
    G = Guard()
    out = nt224(G.new(c.M, c.N), x, w3, bias, c.M, c.N, c.K, w3.stride(1), nseg=c.seg, nseg_stride=w3.stride(0))
    routed = G.new(c.M, c.N)
    with switch("cream_gemm_nt224", 1), tile_launches(1):         # (N = 1344 in segments of 448 at M >= 1024: routed to the tile)
        _check(_lib().cream_linear_fwd_seg(_p(routed), _p(x), _p(w3), _p(bias), c.M, c.N, c.K, w3.stride(1), c.seg, w3.stride(0),
                                           _stream()), "cream_linear_fwd_seg")
    G.check()
    for name, got in (("direct", out), ("routed", routed)):
        _finite(name, got)
        assert torch.equal(got.cpu(), R.ref_fwd_seg(o)), name


@pytest.mark.parametrize("seg", [320, 448])
def test_dgrad_contraction_segments_are_exact_direct_and_routed(seg):
    """qkv dgrad at E = 448: the contraction 3 x seg in segments on the transposed [q | k | v] copies; the same bits from
    cream_linear_nt224 and from cream_linear_dgrad_seg with the switch on (N = 448, M >= 1024: routed to the tile)."""
    lib = _lib()
    c = R.Case(1032, 3 * seg, 448, seg=seg)
    o = R.operands(c, 0)
    dy, wt3 = o.dy.to(DEV)[:c.M], o.wt3.to(DEV)
    G = Guard()
    direct = nt224(G.new(c.M, c.K), dy, wt3, None, c.M, c.K, c.N, wt3.stride(1), kseg=seg, kseg_stride=wt3.stride(0))
    routed = G.new(c.M, c.K)
    with switch("cream_gemm_nt224", 1), tile_launches(1):
        _check(lib.cream_linear_dgrad_seg(_p(routed), _p(dy), _p(wt3), c.M, c.N, c.K, wt3.stride(1), seg, wt3.stride(0), _stream()),
               "cream_linear_dgrad_seg")
    G.check()
    want = R.ref_dgrad_seg(o)
    for name, got in (("direct", direct), ("routed", routed)):
        _finite(name, got)
        assert torch.equal(got.cpu(), want), name


def test_persistent_grids_smaller_than_the_problem_are_exact():
    """5 x 6 = 30 tiles on 8 and on 24 workgroups (several tiles per workgroup, unevenly; the next tile's prefetch before an
    epilogue; the last tile without a successor) and on the whole chip: the same bits."""
    lib = _lib()
    with switch("cream_cu_reserve", 0):
        full = lib.cream_cu_count()
    res = []
    for r in (full - 8, full - 24, 0):
        with switch("cream_cu_reserve", r):
            assert lib.cream_cu_count() == (full - r if r else full)
            res.append(run_exact(R.Case(1032, 1344, 200), R.Case(1032, 200, 1344)))
    for other in res[1:]:
        for k in res[0]:
            assert torch.equal(res[0][k], other[k]), k


def _bound(a, b, K):
    """-> (c, bound): the fp64 product of the bf16 operands; one bf16 rounding of c + fp32 accumulation of K terms."""
    c = a.double() @ b.double().t()
    return c, 2.0 ** -8 * c.abs() + K * 2.0 ** -24 * (a.double().abs() @ b.double().abs().t())


def _ulp_bf16(v):
    """Spacing of bf16 at |v| (fp64 tensor of bf16 values; 0 at 0)."""
    _, e = torch.frexp(v.abs())                                   # |v| = m 2^e, m in [0.5, 1): the leading bit is 2^(e - 1)
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 8))


@pytest.mark.parametrize("M,N,K", [(1032, 448, 448), (1032, 448, 1344)])
def test_random_operands_stay_within_the_derived_bound_and_one_ulp_of_the_other_tiles(M, N, K):
    lib = _lib()
    g = torch.Generator().manual_seed(224 + K)

    def fwd(a, w, on):
        G = Guard()
        out = G.new(M, N)
        with switch("cream_gemm_nt224", on), tile_launches(on):
            _check(lib.cream_linear_fwd(_p(out), _p(a), _p(w), None, M, N, K, K, _stream()), "cream_linear_fwd")
        G.check()
        return out

    # signed operands: the derived bound against fp64, reruns, the routed call = the tile
    a = torch.randn(M, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16)
    ad, wd = a.to(DEV), w.to(DEV)
    c, bound = _bound(a, w, K)
    G = Guard()
    direct = [nt224(G.new(M, N), ad, wd, None, M, N, K, K) for _ in range(2)]
    G.check()
    assert torch.equal(direct[0], direct[1]), "the rerun differs"
    on, off = fwd(ad, wd, 1), fwd(ad, wd, 0)
    assert torch.equal(on, direct[0]), "cream_linear_fwd with the switch on is not the 256 x 224 tile"
    for name, got in (("on", on), ("off", off)):
        err = (got.cpu().double() - c).abs()
        print(f"[nt224 random K={K} switch {name}] max err / bound = {float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), (name, float((err - bound).max()))
    # the switch-off kernel (another contraction order) agrees within one bf16 ulp, element-wise
    on, off = on.cpu().double(), off.cpu().double()
    d = (on - off).abs()
    ulp = _ulp_bf16(torch.maximum(on.abs(), off.abs()))
    print(f"[nt224 random K={K} signed] elements that differ on / off: {int((d > 0).sum())} of {d.numel()}, "
          f"max difference {float((d / ulp.clamp_min(1e-300)).max()):.2f} ulp")
    assert bool((d <= ulp).all())
    # ... and on non-negative operands, where no result is the remainder of a cancellation
    ap, wp = a.abs().to(DEV), w.abs().to(DEV)
    on, off = fwd(ap, wp, 1).cpu().double(), fwd(ap, wp, 0).cpu().double()
    d = (on - off).abs()
    ulp = _ulp_bf16(torch.maximum(on.abs(), off.abs()))
    print(f"[nt224 random K={K} non-negative] elements that differ on / off: {int((d > 0).sum())} of {d.numel()}, "
          f"max difference {float((d / ulp.clamp_min(1e-300)).max()):.2f} ulp")
    assert bool((d <= ulp).all())


def test_routing_reaches_the_tile_exactly_where_the_rule_says():
    """launch_nt: plain and bias epilogues, M >= 1024, N == 448 for every K, N == 1344 with the bias epilogue in segments of 448."""
    lib = _lib()
    z = lambda *shape: torch.zeros(*shape, device=DEV, dtype=BF16)

    def fwd(M, N, K):
        _check(lib.cream_linear_fwd(_p(z(M, N)), _p(z(M, K)), _p(z(N, K)), _p(z(N)), M, N, K, K, _stream()), "cream_linear_fwd")

    def dgrad(M, width, contraction):
        _check(lib.cream_linear_dgrad(_p(z(M, width)), _p(z(M, contraction)), _p(z(width, contraction)), M, contraction, width,
                                      contraction, _stream()), "cream_linear_dgrad")

    def qkv(M, seg, K):
        _check(lib.cream_linear_fwd_seg(_p(z(M, 3 * seg)), _p(z(M, K)), _p(z(3, seg, K)), _p(z(3 * seg)), M, 3 * seg, K, K, seg,
                                        seg * K, _stream()), "cream_linear_fwd_seg")

    with switch("cream_gemm_nt224", 1):
        for K in (320, 448, 1344, 1568, 1792):
            with tile_launches(2):
                fwd(1032, 448, K)
                dgrad(1032, 448, K)
        with tile_launches(1):
            qkv(1032, 448, 384)
        with tile_launches(0):
            fwd(1016, 448, 448)                                   # M < 1024
            dgrad(1016, 448, 448)
            fwd(1032, 384, 448)                                   # other widths
            fwd(1032, 456, 448)
            fwd(1032, 1344, 448)                                  # N = 1344 in ONE segment
            qkv(1032, 384, 448)
    with switch("cream_gemm_nt224", 0), tile_launches(0):
        fwd(1032, 448, 448)
        dgrad(1032, 448, 448)
        qkv(1032, 448, 384)
    torch.cuda.synchronize()
