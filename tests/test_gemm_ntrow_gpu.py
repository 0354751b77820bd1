"""The full-row 256 x E NT tile for the backward's input gradients (csrc/gemm_ntrow.hpp; launch_ntrow, cream_gemm_ntrow and
cream_linear_ntrow in csrc/gemm_mfma.hip).

launch_nt routes the plain-store products (cream_linear_dgrad, cream_linear_dgrad_seg) whose output is exactly 384 or 320 wide
at M >= 1024 to the tile while cream_gemm_ntrow is on.  The tile keeps the contraction order of the tiles it replaces (16
K-elements per MFMA, ascending K), so for every case:
  (a) random normal operands: the routed result equals the switch-off result element for element (torch.equal);
  (b) exact operands (tests/gemm_exact_ref.py: ternary x a power of two, NaN outside the active blocks): bit for bit the fp64
      reference;
  (c) cream_gemm_ntrow_launches rises by one per routed call — and not for M = 512, N = 448, N = 256 or cream_linear_fwd;
  (d) NaN guard bands around the output stay NaN: bands in front of and behind the routed outputs (their row stride is the
      width), and rows above / below plus columns left / right of an output with a row stride larger than its width through
      cream_linear_ntrow, which must give the routed bits.
Shapes: M in 1024 (four full panels) / 1221 (1024 + 197: a ragged last panel) / 1280 (five panels); output width 320 / 384;
contraction 64 (one K-step) / 72 (a zero-filled tail of 8) / 320 (five K-steps) / 1344 (the real depth); a contraction of
3 x width in segments of the width with a segment stride (cream_linear_dgrad_seg); weight rows longer than the active block
(every exact case: ldwt = contraction + 64; one random case).
The CU budget cannot go below 8 (cream_cu_count), so five panels never share a workgroup; M = 2309 (ten panels, the last one
5 rows) on 8 CUs does that: two workgroups walk two panels each — a full panel's epilogue with the next panel's first K-step
in flight, and a ragged last panel behind a full one.  M = 1280 still runs on that 8-CU budget.  The switch and the CU budget
are restored."""
import contextlib
import ctypes

import pytest
import torch

import gemm_exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16

MS = [1024, 1221, 1280]
WIDTHS = [320, 384]
CONTRACTIONS = [64, 72, 320, 1344]
PAD = 4096                                      # elements of NaN in front of and behind a routed output


def _lib():
    from cream_amd import _lib as L
    return L.load()


def _check(rc, what):
    from cream_amd import _lib as L
    L.check(rc, what)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(autouse=True)
def _switches_restored():
    lib = _lib()
    before = (lib.cream_gemm_ntrow(-1), lib.cream_cu_reserve(-1))
    yield
    lib.cream_gemm_ntrow(before[0])
    lib.cream_cu_reserve(before[1])


@contextlib.contextmanager
def switch(name, value):
    fn = getattr(_lib(), name)
    was = fn(value)
    try:
        yield
    finally:
        fn(was)


@contextlib.contextmanager
def tile_launches(n):
    lib = _lib()
    before = lib.cream_gemm_ntrow_launches()
    yield
    got = lib.cream_gemm_ntrow_launches() - before
    assert got == n, f"{got} launches of the full-row tile, expected {n}"


@contextlib.contextmanager
def eight_cus():
    """The smallest CU budget there is: persistent grids of 8 workgroups."""
    lib = _lib()
    with switch("cream_cu_reserve", 0):
        full = lib.cream_cu_count()
    with switch("cream_cu_reserve", full - 8):
        assert lib.cream_cu_count() == 8
        yield


class Flat:
    """A routed output (row stride = width) between two bands of NaN."""

    def __init__(self, M, W):
        self.buf = torch.full((PAD + M * W + PAD,), float("nan"), device=DEV, dtype=BF16)
        self.n = M * W
        self.out = self.buf[PAD:PAD + self.n].view(M, W)

    def check(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:PAD]).all()) and bool(torch.isnan(self.buf[PAD + self.n:]).all()), \
            "the kernel wrote outside its output"
        assert bool(torch.isfinite(self.out).all()), "NaN / inf in the output: a read past K, N or M (the poison) or a lost store"


class Framed:
    """An output with a row stride larger than its width: 8 rows of NaN above and below, 8 + 16 columns left and right."""
    TOP, LEFT, RIGHT = 8, 8, 16

    def __init__(self, M, W):
        self.ld = self.LEFT + W + self.RIGHT
        self.buf = torch.full((M + 2 * self.TOP, self.ld), float("nan"), device=DEV, dtype=BF16)
        self.out = self.buf[self.TOP:self.TOP + M, self.LEFT:self.LEFT + W]

    def check(self):
        torch.cuda.synchronize()
        outside = torch.ones_like(self.buf, dtype=torch.bool)
        outside[self.TOP:self.TOP + self.out.shape[0], self.LEFT:self.LEFT + self.out.shape[1]] = False
        assert bool(torch.isnan(self.buf[outside]).all()), "the kernel wrote into the frame around its output"
        assert bool(torch.isfinite(self.out).all()), "NaN / inf in the output"


def dgrad(out, dy, wt, M, C, W, ldwt):
    """out (M x W) = dy (M x C) . wt (W x C, row stride ldwt)^T through cream_linear_dgrad (N = contraction, K = width)."""
    _check(_lib().cream_linear_dgrad(_p(out), _p(dy), _p(wt), M, C, W, ldwt, _stream()), "cream_linear_dgrad")


def direct(fr, dy, ldx, wt, M, C, W, ldwt, kseg=0, kseg_stride=0):
    _check(_lib().cream_linear_ntrow(_p(fr.out), fr.ld, _p(dy), ldx, _p(wt), M, W, C, ldwt, kseg, kseg_stride, _stream()),
           "cream_linear_ntrow")


def _random(M, C, W, ldwt, seed):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(M, C, generator=g).to(BF16).to(DEV)
    wt = torch.full((W, ldwt), float("nan"), dtype=BF16)
    wt[:, :C] = (torch.randn(W, C, generator=g) * C ** -0.5).to(BF16)
    return dy, wt.to(DEV)


def run_case(M, W, C):
    """(a) - (d) for one shape under the current CU budget."""
    # (a) random normal operands: on == off, element for element
    dy, wt = _random(M, C, W, C, 7 * M + 3 * W + C)
    res = {}
    for on in (1, 0):
        f = Flat(M, W)
        with switch("cream_gemm_ntrow", on), tile_launches(on):                           # (c)
            dgrad(f.out, dy, wt, M, C, W, C)
        f.check()                                                                         # (d)
        res[on] = f.out
    assert torch.equal(res[1], res[0]), "the full-row tile and the switch-off route differ on random operands"
    # (b) exact operands against the fp64 reference; the weight rows are 64 longer than the active block, NaN behind it
    c = R.Case(M, C, W)
    o = R.operands(c, 0)
    dyx, wtx = o.dy.to(DEV), o.wt.to(DEV)
    want = R.ref_dgrad(o)
    f = Flat(M, W)
    with switch("cream_gemm_ntrow", 1), tile_launches(1):
        dgrad(f.out, dyx, wtx, M, C, W, wtx.stride(0))
    f.check()
    assert torch.equal(f.out.cpu(), want), R.case_id(c)
    # (d) rows and columns around an output with its own row stride
    fr = Framed(M, W)
    with tile_launches(1):
        direct(fr, dyx, dyx.stride(0), wtx, M, C, W, wtx.stride(0))
    fr.check()
    assert torch.equal(fr.out.cpu(), want), R.case_id(c)


@pytest.mark.parametrize("C", CONTRACTIONS)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("M", MS)
def test_routed_input_gradients_are_the_switch_off_bits_and_exact(M, W, C):
    if M == 1280:
        with eight_cus():
            run_case(M, W, C)
    else:
        run_case(M, W, C)


@pytest.mark.parametrize("C", [72, 320])
@pytest.mark.parametrize("W", WIDTHS)
def test_two_panels_per_workgroup_on_eight_cus(W, C):
    with eight_cus():
        run_case(2309, W, C)


@pytest.mark.parametrize("W", WIDTHS)
def test_contraction_segments_with_a_segment_stride(W):
    """qkv input gradient at E / 64 heads: the contraction 3 x W in segments of W on the transposed [q | k | v] copies."""
    lib = _lib()
    c = R.Case(1221, 3 * W, W, seg=W)
    o = R.operands(c, 0)
    dy, wt3 = o.dy.to(DEV), o.wt3.to(DEV)                                # wt3: (3, ldw, W + 64)
    want = R.ref_dgrad_seg(o)
    assert wt3.stride(0) > W * wt3.stride(1) > W * W

    def seg_call(out):
        _check(lib.cream_linear_dgrad_seg(_p(out), _p(dy), _p(wt3), c.M, c.N, c.K, wt3.stride(1), W, wt3.stride(0), _stream()),
               "cream_linear_dgrad_seg")

    res = {}
    for on in (1, 0):
        f = Flat(c.M, W)
        with switch("cream_gemm_ntrow", on), tile_launches(on):
            seg_call(f.out)
        f.check()
        assert torch.equal(f.out.cpu(), want), f"switch {on}"
        res[on] = f.out
    assert torch.equal(res[1], res[0])
    fr = Framed(c.M, W)
    with tile_launches(1):
        direct(fr, dy, dy.stride(0), wt3, c.M, c.N, W, wt3.stride(1), kseg=W, kseg_stride=wt3.stride(0))
    fr.check()
    assert torch.equal(fr.out.cpu(), want)
    # random operands in the same layout: on == off
    g = torch.Generator().manual_seed(3 * W)
    dyr = torch.randn(c.M, 3 * W, generator=g).to(BF16).to(DEV)
    wtr = (torch.randn(3, W, W + 64, generator=g) * (3 * W) ** -0.5).to(BF16).to(DEV)
    res = {}
    for on in (1, 0):
        f = Flat(c.M, W)
        with switch("cream_gemm_ntrow", on), tile_launches(on):
            _check(lib.cream_linear_dgrad_seg(_p(f.out), _p(dyr), _p(wtr), c.M, c.N, c.K, wtr.stride(1), W, wtr.stride(0),
                                              _stream()), "cream_linear_dgrad_seg")
        f.check()
        res[on] = f.out
    assert torch.equal(res[1], res[0])


@pytest.mark.parametrize("W", WIDTHS)
def test_weight_rows_longer_than_the_contraction_on_random_operands(W):
    M, C = 1221, 328
    dy, wt = _random(M, C, W, C + 24, 11 * W)
    res = {}
    for on in (1, 0):
        f = Flat(M, W)
        with switch("cream_gemm_ntrow", on), tile_launches(on):
            dgrad(f.out, dy, wt, M, C, W, C + 24)
        f.check()
        res[on] = f.out
    assert torch.equal(res[1], res[0])


def test_routing_reaches_the_tile_exactly_where_the_rule_says():
    """launch_nt: plain-store epilogue, M >= 1024, N == 384 or 320, switch on."""
    lib = _lib()
    z = lambda *shape: torch.zeros(*shape, device=DEV, dtype=BF16)

    def dg(M, W, C):
        dgrad(z(M, W), z(M, C), z(W, C), M, C, W, C)

    def fwd(M, N, K):
        _check(lib.cream_linear_fwd(_p(z(M, N)), _p(z(M, K)), _p(z(N, K)), _p(z(N)), M, N, K, K, _stream()), "cream_linear_fwd")

    with switch("cream_gemm_ntrow", 1):
        with tile_launches(2):
            dg(1024, 384, 64)
            dg(1032, 320, 960)
        with tile_launches(0):
            dg(512, 384, 64)                                     # M < 1024
            dg(1016, 320, 64)
            dg(1032, 448, 64)                                    # other widths
            dg(1032, 256, 64)
            fwd(1032, 384, 64)                                   # bias epilogue
            fwd(1032, 320, 448)
    with switch("cream_gemm_ntrow", 0), tile_launches(0):
        dg(1032, 384, 64)
        dg(1032, 320, 64)
    torch.cuda.synchronize()
