"""Bit-exact tests of the hand-written MFMA GEMMs (csrc/gemm_mfma.hpp, gemm_nt8.hpp, gemm_tn8.hpp, launchers in gemm_mfma.hip) on
operands for which they MUST be exact (tests/gemm_exact_ref.py: ternary x a power of two, every result an integer <= 256 in its
unit, so fp32 accumulation in any order and the bf16 output are exact): the kernel output equals the fp64 CPU reference bit for
bit whatever the tile, split, epilogue schedule or grid.  Every kernel family is forced through the library's own switches (see
launch_nt in csrc/gemm_mfma.hip; the table is NT_FAMILIES in gemm_exact_ref.py) and every switch is restored.

What is swept:
  * K tails per NT family: the contraction 64 q + r for every r in 8 .. 56 and 8 / 24 / 56 / 64 / 72 / 120 / 128 (zero, one, two
    K-steps; 1152 + r for the 256 x 256 two-stage tile in its default mode), under all four epilogues (bias, bias + GELU contract
    over K; plain store and x gelu' with column sums contract over N), ntopt 0 / 3 / 11 on the two-stage 128-wide tiles;
  * token tails of both TN kernels (M = 8 .. 600, tiles that stick out of the matrix both ways), bf16 and fp32 partials;
  * row edges M = 1, 8, 127, 129, 600, 1032 per family;
  * supernet-T / -B shapes at M = 600 with the library's defaults and again with cream_gemm_nt8(1).  One (E, Q, F) choice per
    distinct (K % 64, N % 256) class — T: E 192 / 216 / 240 with Q 192, 256 and F 672, 768 / 760 (756 padded), 864 / 840, 960;
    B: E 528 with Q 512, 576 and F 1584, 1848, 2112; E 576 with Q 576, 640 and F 1728, 2016, 2304; E 624 with Q 512, 640 and
    F 1872, 2184, 2496 — qkv with segment addressing (forward and dgrad), proj, fc1 + GELU, fc2, x gelu' with its column sums, all
    four weight gradients;
  * persistent grids smaller than the problem: cream_cu_reserve leaving 8 and 24 CUs, and 0 — bit-identical across the budgets.
Not exact by construction, with derived bounds: gelu / gelu' values (one bf16 ulp + the erf approximation's 1e-6) and the
fp32 column-sum partials (M x 2^-23 x sum |dh|)."""
import contextlib
import ctypes
from functools import lru_cache

import pytest
import torch

import gemm_exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16

_SWITCH = dict(nt8="cream_gemm_nt8", nt256="cream_gemm_nt256", nthalf="cream_gemm_nthalf", ntopt="cream_gemm_ntopt",
               tn8="cream_gemm_tn8", wgrad_bf16="cream_block_wgrad_bf16", reserve="cream_cu_reserve")


def _lib():
    from cream_amd import _lib as L
    return L.load()


@contextlib.contextmanager
def switches(**kw):
    """Sets process-global switches of the library and puts back what each call returned."""
    lib, was = _lib(), []
    try:
        for k, v in kw.items():
            fn = getattr(lib, _SWITCH[k])
            was.append((fn, fn(v)))
        yield
    finally:
        for fn, w in reversed(was):
            fn(w)


@pytest.fixture(scope="module", autouse=True)
def _switches_untouched():
    lib = _lib()
    before = {k: getattr(lib, n)(-1) for k, n in _SWITCH.items()}
    yield
    after = {k: getattr(lib, n)(-1) for k, n in _SWITCH.items()}
    for k, n in _SWITCH.items():
        getattr(lib, n)(before[k])
    assert after == before, (before, after)


class Guard:
    """Outputs as views into buffers filled with -7 with a guard band behind them."""

    def __init__(self):
        self.bufs = []

    def new(self, *shape, dtype=BF16):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 4096,), -7.0, device=DEV, dtype=dtype)
        self.bufs.append((buf, n))
        return buf[:n].view(*shape)

    def check(self):
        for buf, n in self.bufs:
            assert bool((buf[n:] == -7).all()), "a kernel wrote behind its output"


class Dev:
    """The operands of a case on the device + lazily computed CPU references."""

    def __init__(self, case):
        self.case, self.o = case, R.operands(case, 0)
        o = self.o
        for name in ("x", "dy", "factor", "bias", "bias_gelu", "wsup", "wt") + (("w3", "wt3") if case.seg else ()):
            setattr(self, name, getattr(o, name).to(DEV))
        self._ref = {}

    def ref(self, what):
        if what not in self._ref:
            o = self.o
            self._ref[what] = {"out": lambda: R.ref_fwd(o), "out0": lambda: R.ref_fwd(o, False), "gelu": lambda: R.ref_gelu(o),
                               "dx": lambda: R.ref_dgrad(o), "dh": lambda: R.ref_dgrad_mul(o)[0], "seg": lambda: R.ref_fwd_seg(o),
                               "dx_seg": lambda: R.ref_dgrad_seg(o), "wgrad": lambda: R.ref_wgrad(o),
                               "bsum": lambda: R.ref_colsum_dy(o)}[what]()
        return self._ref[what]


@lru_cache(maxsize=3)
def dev(case):
    return Dev(case)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def run_fwd_type(d):
    """The products that contract over K: bias / no bias (+ segment addressing), bias + GELU (both outputs; g only)."""
    from cream_amd import _lib as L
    from cream_amd.autoformer import block as K_
    c, G = d.case, Guard()
    M, N, K = c.M, c.N, c.K
    x = d.x[:M]
    res = dict(out=K_.linear_fwd(x, d.wsup, d.bias, N, K, out=G.new(M, N)),
               out0=K_.linear_fwd(x, d.wsup, None, N, K, out=G.new(M, N)))
    if c.seg:
        res["seg"] = K_.linear_fwd_seg(x, d.w3, d.bias, N, K, c.seg, out=G.new(M, N))
    if c.nvalid:
        lib, st = L.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        gp, g, g2 = G.new(M, N), G.new(M, N), G.new(M, N)
        L.check(lib.cream_linear_gelu_fwd_pad(_ptr(gp), _ptr(g), _ptr(x), _ptr(d.wsup), _ptr(d.bias_gelu), M, N, c.nvalid, K,
                                              d.wsup.stride(0), st), "cream_linear_gelu_fwd_pad")
        L.check(lib.cream_linear_gelu_fwd_pad(None, _ptr(g2), _ptr(x), _ptr(d.wsup), _ptr(d.bias_gelu), M, N, c.nvalid, K,
                                              d.wsup.stride(0), st), "cream_linear_gelu_fwd_pad")
        res.update(gp=gp, g=g, g_only=g2)
    else:
        res["gp"], res["g"] = K_.linear_gelu_fwd(x, d.wsup, d.bias_gelu, N, K)
        none, res["g_only"] = K_.linear_gelu_fwd(x, d.wsup, d.bias_gelu, N, K, want_grad=False)
        assert none is None
    torch.cuda.synchronize()
    G.check()
    return res


def run_bwd_type(d):
    """The products that contract over N: dgrad (+ segment addressing), (dy . W) x factor with its column-sum partials."""
    from cream_amd.autoformer import block as K_
    c, G = d.case, Guard()
    M, N, K = c.M, c.N, c.K
    dy = d.dy[:M]
    res = dict(dx=K_.linear_dgrad(dy, d.wt, N, K, out=G.new(M, K)))
    if c.seg:
        res["dx_seg"] = K_.linear_dgrad_seg(dy, d.wt3, N, K, c.seg, out=G.new(M, K))
    res["dh"], res["cs"] = K_.linear_dgrad_mul(dy, d.wt, d.factor[:M], N, K)
    torch.cuda.synchronize()
    G.check()
    return res


def run_tn(d):
    """Weight gradients: the macro-tile kernel (bf16 partials at the library's S), the 128 x 128 kernel at the same S, and the
    fp32-partials entry point; bias partials ride along."""
    from cream_amd.autoformer import block as K_
    c, G, lib = d.case, Guard(), _lib()
    M, N, K = c.M, c.N, c.K
    dy, x = d.dy[:M], d.x[:M]
    with switches(tn8=2):
        S = lib.cream_linear_wgrad_splits_bf16(M, N, K)
        assert S >= 1
        p8, b8 = K_.linear_wgrad_parts(dy, x, want_bias=True, out=G.new(S, N, K), bias_out=G.new(S, N, dtype=torch.float32))
        p8n, none = K_.linear_wgrad_parts(dy, x, want_bias=False, out=G.new(S, N, K))
        assert none is None
    with switches(tn8=0):
        p1, b1 = K_.linear_wgrad_parts(dy, x, want_bias=True, out=G.new(S, N, K), bias_out=G.new(S, N, dtype=torch.float32))
    S32 = lib.cream_linear_wgrad_splits(M, N, K)
    p32, b32 = K_.linear_wgrad_parts(dy, x, want_bias=True, out=G.new(S32, N, K, dtype=torch.float32),
                                     bias_out=G.new(S32, N, dtype=torch.float32))
    torch.cuda.synchronize()
    G.check()
    return dict(S=S, tn8=p8, tn8_bias=b8, tn8_nobias=p8n, tn128=p1, tn128_bias=b1, fp32=p32, fp32_bias=b32)


def _finite(name, t):
    assert bool(torch.isfinite(t).all()), f"{name}: NaN / inf — a read past K, N or M (the poison) or a lost store"


def check_fwd_type(d, res):
    c = d.case
    for k, v in res.items():
        _finite(k, v)
    assert torch.equal(res["out"].cpu(), d.ref("out")), "bias epilogue"
    assert torch.equal(res["out0"].cpu(), d.ref("out0")), "forward without bias"
    if c.seg:
        assert torch.equal(res["seg"].cpu(), d.ref("seg")), "segment-addressed forward"
    h, g, gp = d.ref("gelu")
    hd = h.double()
    for name, got, want in (("gelu", res["g"], g), ("gelu'", res["gp"], gp)):
        err = (got.cpu().double() - want).abs()
        assert bool((err <= R.gelu_bound(want, hd)).all()), (name, float((err - R.gelu_bound(want, hd)).max()))
    assert torch.equal(res["g_only"], res["g"]), "want_grad=False writes the same g"
    if c.nvalid:
        assert float(res["g"][:, c.nvalid:].abs().max()) == 0.0 and float(res["gp"][:, c.nvalid:].abs().max()) == 0.0


def check_bwd_type(d, res):
    c = d.case
    for k, v in res.items():
        _finite(k, v)
    assert torch.equal(res["dx"].cpu(), d.ref("dx")), "dgrad"
    if c.seg:
        assert torch.equal(res["dx_seg"].cpu(), d.ref("dx_seg")), "segment-addressed dgrad"
    dh = d.ref("dh")
    assert torch.equal(res["dh"].cpu(), dh), "(dy . W) x factor: one rounding of an exact product"
    cs = res["cs"].cpu().double()
    assert cs.shape == (_lib().cream_colsum128_slabs(c.M), c.K)
    bound = c.M * 2.0 ** -23 * dh.double().abs().sum(0)                       # fp32 summation of M terms
    assert bool(((cs.sum(0) - dh.double().sum(0)).abs() <= bound).all()), "column-sum partials"


def check_tn(d, res):
    c, S = d.case, res["S"]
    for k, v in res.items():
        if k != "S":
            _finite(k, v)
    want = R.ref_wgrad_parts(d.o, S)
    for name in ("tn8", "tn8_nobias", "tn128"):
        got = res[name].cpu()
        for s in range(S):
            assert torch.equal(got[s], want[s]), (name, s, R.wgrad_slices(c.M, S)[s])
    assert torch.equal(res["fp32"].cpu().double().sum(0), d.ref("wgrad")), "fp32 partials add up exactly"
    for name in ("tn8_bias", "tn128_bias", "fp32_bias"):
        assert torch.equal(res[name].cpu().double().sum(0), d.ref("bsum")), name


def _same(a, b, what, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k in skip:
            continue
        if k == "S":
            assert a[k] == b[k]
        else:
            assert torch.equal(a[k], b[k]), (what, k)


def twice(run, check, d, what):
    """Runs all entry points on one set of operands twice: equal to the reference, the rerun bit-identical."""
    a = run(d)
    check(d, a)
    b = run(d)
    _same(a, b, what + ": rerun")
    return a


def nt_family(fam, M, contraction):
    """Both orientations of a contraction length under the family's switches (and ntopt values)."""
    sw, W, _, _, ntopts = R.NT_FAMILIES[fam]
    fwd_case, bwd_case = R.sweep_pair(W, M, contraction)
    first = None
    for opt in ntopts:
        kw = dict(sw, ntopt=opt) if (len(ntopts) > 1) else dict(sw)
        with switches(**kw):
            res = (twice(run_fwd_type, check_fwd_type, dev(fwd_case), f"{fam} ntopt {opt}"),
                   twice(run_bwd_type, check_bwd_type, dev(bwd_case), f"{fam} ntopt {opt}"))
        if first is None:
            first = res
        else:                                   # the epilogue schedules agree bit for bit (gelu / gelu' included)
            _same(first[0], res[0], f"{fam}: ntopt {ntopts[0]} vs {opt}")
            _same(first[1], res[1], f"{fam}: ntopt {ntopts[0]} vs {opt}")


@pytest.mark.parametrize("fam,contraction", R.TAIL_CASES, ids=[f"{f}-k{c}" for f, c in R.TAIL_CASES])
def test_contraction_tails_are_exact_in_every_nt_family(fam, contraction):
    nt_family(fam, R.NT_FAMILIES[fam][2], contraction)


@pytest.mark.parametrize("fam,M", R.ROW_CASES, ids=[f"{f}-M{m}" for f, m in R.ROW_CASES])
def test_row_edges_are_exact_in_every_nt_family(fam, M):
    nt_family(fam, M, R._row_contraction(fam))


@pytest.mark.parametrize("case", R.TN_CASES, ids=R.case_id)
def test_token_tails_are_exact_in_both_tn_kernels(case):
    twice(run_tn, check_tn, dev(case), "TN")


@pytest.mark.parametrize("case", R.SPACE_CASES, ids=R.case_id)
def test_search_space_shapes_are_exact(case):
    """Supernet-T / -B products at M = 600 through whatever kernel the library picks with its defaults, and with gemm_nt8
    wherever its limits allow."""
    d = dev(case)
    a = (twice(run_fwd_type, check_fwd_type, d, "defaults"), twice(run_bwd_type, check_bwd_type, d, "defaults"))
    twice(run_tn, check_tn, d, "defaults")
    with switches(nt8=1):
        b = (twice(run_fwd_type, check_fwd_type, d, "nt8"), twice(run_bwd_type, check_bwd_type, d, "nt8"))
    _same(a[0], b[0], "defaults vs nt8")
    _same(a[1], b[1], "defaults vs nt8", skip=("cs",))       # (the fp32 column-sum partials: another summation order, bounded in check_bwd_type)


def _budgets():
    """cream_cu_reserve values that leave 8 and 24 CUs, and 0 (computed from the count at reserve 0)."""
    lib = _lib()
    with switches(reserve=0):
        full = lib.cream_cu_count()
    return full, [full - 8, full - 24, 0]


@pytest.mark.parametrize("fam,fwd_case,bwd_case", R.GRID_CASES, ids=[g[0] for g in R.GRID_CASES])
def test_persistent_grids_smaller_than_the_problem_are_exact(fam, fwd_case, bwd_case):
    """Several tiles per workgroup, unevenly: the next tile's prefetch before an epilogue, the K-tile stream across a tile boundary,
    the last tile without a successor — same bits at every CU budget."""
    lib = _lib()
    sw = R.NT_FAMILIES[fam][0]
    full, reserves = _budgets()
    res = []
    for r in reserves:
        with switches(reserve=r, **sw):
            assert lib.cream_cu_count() == (full - r if r else full)
            res.append((twice(run_fwd_type, check_fwd_type, dev(fwd_case), f"{fam} reserve {r}"),
                        twice(run_bwd_type, check_bwd_type, dev(bwd_case), f"{fam} reserve {r}")))
    for r, other in zip(reserves[1:], res[1:]):
        _same(res[0][0], other[0], f"{fam}: 8 CUs vs reserve {r}")
        _same(res[0][1], other[1], f"{fam}: 8 CUs vs reserve {r}")


def test_token_slices_of_the_weight_gradient_follow_the_cu_budget_and_stay_exact():
    d = dev(R.GRID_TN_CASE)
    full, reserves = _budgets()
    S = {}
    for r in reserves:
        with switches(reserve=r):
            res = twice(run_tn, check_tn, d, f"TN reserve {r}")
            S[r] = res["S"]
            total = res["tn8"].cpu().double().sum(0)
        assert torch.equal(total, d.ref("wgrad"))
    print(f"[weight-gradient token slices of {R.case_id(R.GRID_TN_CASE)}] " + ", ".join(f"{full - r} CUs: S = {s}" for r, s in S.items()))
    assert S[0] != S[full - 8], "the split count did not follow the budget: the case tests nothing"
