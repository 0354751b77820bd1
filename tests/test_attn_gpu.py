"""GPU parity of the fused attention kernels (cream_attn_rpe2d_fwd / _bwd, called through the
C ABI) against the oracle's dense restatement of multihead_super.py:135-154 and its autograd:
fp32 within 1e-3 relative (BASELINE.json's bar; measured ~1e-6), bf16 within the documented
2e-2; plus size-independent properties at the benchmark's full size."""
import pytest
import torch

from oracle import autoformer_oracle as AO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _inputs(B, H, side, mr, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = side * side + 1
    qkv = torch.randn(B, N, 3, H, 64, generator=g)
    tabs = [torch.randn(2 * mr + 2, 64, generator=g) * 0.5 for _ in range(4)]
    go = torch.randn(B, N, H, 64, generator=g)
    return qkv, tabs, go


def _oracle(qkv, tabs, go, mr):
    x = [qkv.clone().requires_grad_()] + [t.clone().requires_grad_() for t in tabs]
    out = AO.attention_core(x[0], *x[1:], 0.125, mr)
    out.backward(go)
    return out.detach(), [t.grad for t in x]


def _fused(qkv, tabs, go, mr, dtype):
    from cream_amd.autoformer import fused_attention as FA
    x = [qkv.to(DEV, dtype).requires_grad_()] + [t.to(DEV).requires_grad_() for t in tabs]
    out = FA.attention_rpe2d_fused(x[0], *x[1:], 0.125, mr)
    out.backward(go.to(DEV, dtype))
    return out.detach(), [t.grad for t in x]


# (B, H, side, max_rel): the benchmark geometry, a small grid, the 8-tile kernel, clamping
# active (side-1 > max_rel), the smallest grid, and a non-multiple-of-4 head count
CASES = [(2, 3, 14, 14), (1, 2, 7, 14), (1, 1, 15, 14), (1, 2, 5, 3), (2, 1, 1, 14), (1, 5, 9, 4)]


@pytest.mark.parametrize("B,H,side,mr", CASES)
def test_fused_attention_fp32_matches_oracle(B, H, side, mr):
    qkv, tabs, go = _inputs(B, H, side, mr)
    ref_out, ref_g = _oracle(qkv, tabs, go, mr)
    out, g = _fused(qkv, tabs, go, mr, torch.float32)
    assert _rel(out, ref_out) < 1e-3
    for a, b in zip(g, ref_g):
        assert _rel(a, b) < 1e-3


@pytest.mark.parametrize("B,H,side,mr", CASES[:4])
def test_fused_attention_bf16_documented_tolerance(B, H, side, mr):
    qkv, tabs, go = _inputs(B, H, side, mr, seed=1)
    ref_out, ref_g = _oracle(qkv, tabs, go, mr)
    out, g = _fused(qkv, tabs, go, mr, torch.bfloat16)
    assert _rel(out, ref_out) < 2e-2
    for a, b in zip(g, ref_g):
        assert _rel(a, b) < 3e-2


def test_fused_equals_bucketed_hip_path():
    """Two independent HIP executions of the same algebra (rpe_index gather/scatter kernels +
    library GEMMs vs the fused kernels)."""
    from cream_amd.autoformer import attention_op
    from cream_amd.autoformer.modules import relative_index_tables
    qkv, tabs, go = _inputs(2, 3, 14, 14, seed=2)
    iv, ih = relative_index_tables(197, 14, DEV)
    outs = {}
    for impl in ("fused", "bucketed"):
        x = [qkv.to(DEV).requires_grad_()] + [t.to(DEV).requires_grad_() for t in tabs]
        out = attention_op.attention_rpe2d(x[0], *x[1:], iv, ih, 0.125, impl=impl, max_relative_position=14)
        out.backward(go.to(DEV))
        outs[impl] = (out.detach(), [t.grad for t in x])
    assert _rel(outs["fused"][0], outs["bucketed"][0]) < 1e-5
    for a, b in zip(outs["fused"][1], outs["bucketed"][1]):
        assert _rel(a, b) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_size_properties(dtype):
    """BASELINE size (B=128, H=6, N=197): rows of P sum to one, the output is linear in V and
    in the value tables, and both directions are bit-reproducible (no atomics)."""
    from cream_amd.autoformer import fused_attention as FA
    B, H, N, mr = 128, 6, 197, 14
    g = torch.Generator(device=DEV).manual_seed(3)
    qkv = torch.randn(B, N, 3, H, 64, device=DEV, generator=g).to(dtype)
    tabs = [torch.randn(30, 64, device=DEV, generator=g) * 0.5 for _ in range(4)]
    zero = torch.zeros(30, 64, device=DEV)
    # (1) V = 1, value tables = 0  ->  O = sum_j P = 1
    q1 = qkv.clone()
    q1[:, :, 2] = 1
    out = FA.attention_rpe2d_fused(q1, tabs[0], tabs[1], zero, zero, 0.125, mr)
    assert float((out.float() - 1).abs().max()) < (1e-5 if dtype == torch.float32 else 2e-2)
    # (2) V = 0, value tables = const c -> O = c * (sum of bucket weights) = 2c (vertical + horizontal)
    q0 = qkv.clone()
    q0[:, :, 2] = 0
    ones = torch.ones(30, 64, device=DEV)
    out = FA.attention_rpe2d_fused(q0, tabs[0], tabs[1], ones, 0.5 * ones, 0.125, mr)
    assert float((out.float() - 1.5).abs().max()) < (1e-5 if dtype == torch.float32 else 3e-2)
    # (3) bit-reproducible forward and backward
    res = []
    for _ in range(2):
        x = [qkv.clone().requires_grad_()] + [t.clone().requires_grad_() for t in tabs]
        o = FA.attention_rpe2d_fused(x[0], *x[1:], 0.125, mr)
        o.backward(torch.ones_like(o))
        res.append([o.detach()] + [t.grad for t in x])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # (4) the saved log-sum-exp is finite and the gradient of sum(O) w.r.t. q,k vanishes when V and
    # the value tables are constant (P sums to one for any logits)
    x = q1.clone().requires_grad_()
    FA.attention_rpe2d_fused(x, tabs[0], tabs[1], zero, zero, 0.125, mr).float().sum().backward()
    assert float(x.grad[:, :, :2].float().abs().max()) < (1e-4 if dtype == torch.float32 else 5e-2)


def test_c_abi_rejects_bad_arguments():
    import ctypes
    from cream_amd import _lib
    lib = _lib.load()
    q = torch.zeros(1, 5, 3, 1, 64, device=DEV)
    out = torch.zeros(1, 5, 1, 64, device=DEV)
    lse = torch.zeros(1, 1, 5, device=DEV)
    sp = torch.zeros(1, 1, 64, 32, device=DEV)
    t = torch.zeros(30, 64, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    args = lambda N, gh, gw, dt: (p(out), p(lse), p(sp), p(q), p(q), p(q), 960, 192, 64, p(t), p(t), p(t), p(t), 64,
                                  1, 1, N, gh, gw, 14, 0.125, dt, None)
    assert lib.cream_attn_rpe2d_fwd(*args(5, 2, 2, _lib.F32)) == 0
    assert lib.cream_attn_rpe2d_fwd(*args(6, 2, 2, _lib.F32)) == -4          # N != gh*gw + 1
    assert lib.cream_attn_rpe2d_fwd(*args(5, 2, 2, _lib.F16)) == -2          # dtype not supported
    assert lib.cream_attn_rpe2d_fwd(*args(290, 17, 17, _lib.F32)) == -4      # too many tokens / slots
    torch.cuda.synchronize()


@pytest.mark.parametrize("H", [5, 6, 7])
def test_attention_at_bench_batch_matches_oracle(H):
    """cream_attn_rpe2d_fwd/bwd at the benchmarked size (B = 128, N = 197, H = 5/6/7: 640/768/896
    workgroups) against the reference's dense formulation (oracle AO.attention_core, CPU fp32) on the
    same bf16-rounded inputs: output, dq/dk/dv and the four table gradients.  Measured on the MI355X
    (gpurun_out r02i: H=5/6/7): out 3.6/4.1/2.8e-3, dqkv 0.9/1.3/1.7e-2 (bf16 side buffers of the
    two-launch backward), tables 3.9/3.7/3.2e-3 (max-abs / max-abs); bounds = 2x the worst."""
    from cream_amd.autoformer import fused_attention as FA
    from oracle import autoformer_oracle as AO
    g = torch.Generator().manual_seed(H)
    B, N = 128, 197
    qkv = (torch.randn(B, N, 3, H, 64, generator=g) * 0.7).bfloat16()
    tabs = [(torch.randn(30, 64, generator=g) * 0.5) for _ in range(4)]
    do = (torch.randn(B, N, H, 64, generator=g) * 0.5).bfloat16()
    qr = qkv.float().requires_grad_(True)
    tr = [t.clone().requires_grad_(True) for t in tabs]
    out_ref = AO.attention_core(qr, *tr, 0.125, 14)
    out_ref.backward(do.float())
    qd = qkv.to(DEV)
    td = [t.to(DEV) for t in tabs]
    o, lse, sp = FA.attn_fwd_raw(qd, *td, 0.125, 14)
    dqkv, dtab = FA.attn_bwd_raw(do.to(DEV), qd, *td, o, lse, sp, 0.125, 14, reduce_tables=True)
    e_out = _rel(o.float().view(B, N, H, 64), out_ref)
    e_dqkv = _rel(dqkv.float().view(B, N, 3, H, 64), qr.grad)
    e_tab = max(_rel(dtab[i][:30], tr[i].grad) for i in range(4))
    print(f"[B=128 attention H={H}] out {e_out:.1e} dqkv {e_dqkv:.1e} tables {e_tab:.1e}")
    assert e_out < 8.2e-3 and e_dqkv < 3.4e-2 and e_tab < 7.8e-3


@pytest.mark.parametrize("B,H", [(2, 3), (50, 6), (128, 5)])
def test_kernel_variants_of_the_benchmark_geometry_agree(B, H):
    """The AutoFormer geometry (N = 197, bf16) has two backward implementations (one-pass kernel / two-launch pair,
    cream_attn_rpe2d_bwd_mode — the pair is what every other geometry and the fp32 parity mode run): on the same inputs
    the backwards must agree to the reordering of their fp32 sums (one bf16 ulp on dq / dk / dv), a rerun of the one-pass kernel
    bit for bit; items < compute units, items not a multiple of them, and the benchmark batch."""
    from cream_amd import _lib
    lib = _lib.load()
    qkv, tabs, go = _inputs(B, H, 14, 14, seed=B + H)
    res = {}
    prev_b = lib.cream_attn_rpe2d_bwd_mode(-1)
    try:
        for bm in (0, 1, 1):
            lib.cream_attn_rpe2d_bwd_mode(bm)
            res.setdefault(bm, []).append(_fused(qkv, tabs, go, 14, torch.bfloat16))
    finally:
        lib.cream_attn_rpe2d_bwd_mode(prev_b)
    out0, g0 = res[0][0]
    out1, g1 = res[1][0]
    out1b, g1b = res[1][1]
    assert torch.equal(out0, out1) and torch.equal(out1, out1b)             # one forward kernel
    for a, b in zip(g1, g1b):                                               # the one-pass backward is reproducible
        assert torch.equal(a, b)
    for i, (a, b) in enumerate(zip(g1, g0)):                                # one-pass vs two-launch
        assert torch.isfinite(a).all()
        # dqkv (bf16): at most one ulp (2^-8) on the largest elements; the four table gradients (fp32 sums): 2e-3
        assert _rel(a, b) < (8e-3 if i == 0 else 2e-3), (i, _rel(a, b))


@pytest.mark.parametrize("B,H", [(2, 3), (50, 6), (128, 5), (128, 7)])
def test_role_split_backward_equals_the_one_pass_kernel(B, H):
    """csrc/attn_rpe2d_bwd2.hpp (cream_attn_rpe2d_bwd_mode(2), round 6): the one-pass backward with the query-tile owners and
    the key-tile jobs on separate waves (12 waves of <= 168 registers instead of 7 of 238), the table gradients kept in registers
    across a workgroup's items.  dq / dk / dv keep bwd1's contraction order: BIT-IDENTICAL; the table gradients are the same
    products added in one fp32 chain per workgroup instead of per-item chains (= the two-launch kernels' order): 1e-5; a rerun
    reproduces every bit (multihead_super.py:133-160)."""
    from cream_amd import _lib
    lib = _lib.load()
    qkv, tabs, go = _inputs(B, H, 14, 14, seed=3 * B + H)
    res = {}
    prev_b = lib.cream_attn_rpe2d_bwd_mode(-1)
    try:
        for bm in (1, 2, 2):
            lib.cream_attn_rpe2d_bwd_mode(bm)
            res.setdefault(bm, []).append(_fused(qkv, tabs, go, 14, torch.bfloat16))
    finally:
        lib.cream_attn_rpe2d_bwd_mode(prev_b)
    (_, g1), (_, g2), (_, g2b) = res[1][0], res[2][0], res[2][1]
    for a, b in zip(g2, g2b):
        assert torch.equal(a, b)
    assert torch.isfinite(g2[0]).all() and torch.equal(g2[0], g1[0])
    for i in range(1, len(g1)):
        assert torch.isfinite(g2[i]).all() and _rel(g2[i], g1[i]) < 1e-5, (i, _rel(g2[i], g1[i]))


# ---- attention dropout inside the fused kernels (multihead_super.py:145 `attn = self.attn_drop(attn)`) --------------------------
def _keep(seed, p, B, H, N):
    """keep / (1 - p) as the kernels regenerate it (numpy restatement of csrc/attn_common.hpp drop_keep)."""
    from cream_amd import irpe_fused
    import numpy as np
    h = irpe_fused.dropout_keep_mask(seed, B, H, N)
    return torch.from_numpy((h >= np.uint32(irpe_fused.dropout_threshold(p))).astype("float32")) / (1.0 - p)


def _oracle_drop(qkv, tabs, go, mr, keep):
    x = [qkv.clone().requires_grad_()] + [t.clone().requires_grad_() for t in tabs]
    out = AO.attention_core(x[0], *x[1:], 0.125, mr, attn_keep=keep)
    out.backward(go)
    return out.detach(), [t.grad for t in x]


def _fused_drop(qkv, tabs, go, mr, dtype, p, seed):
    from cream_amd.autoformer import fused_attention as FA
    x = [qkv.to(DEV, dtype).requires_grad_()] + [t.to(DEV).requires_grad_() for t in tabs]
    out = FA.attention_rpe2d_fused(x[0], *x[1:], 0.125, mr, dropout_p=p, seed=seed)
    out.backward(go.to(DEV, dtype))
    return out.detach(), [t.grad for t in x]


@pytest.mark.parametrize("B,H,side,mr", CASES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_fused_attention_dropout_fp32_matches_oracle_under_the_same_mask(B, H, side, mr, p):
    """Every geometry of the kernel family with attn_drop > 0: outputs and all five gradients against the dense
    restatement evaluated under the mask the kernels regenerate from the seed."""
    qkv, tabs, go = _inputs(B, H, side, mr, seed=5)
    keep = _keep(1234 + side, p, B, H, side * side + 1)
    ref_out, ref_g = _oracle_drop(qkv, tabs, go, mr, keep)
    out, g = _fused_drop(qkv, tabs, go, mr, torch.float32, p, 1234 + side)
    assert _rel(out, ref_out) < 1e-3
    for a, b in zip(g, ref_g):
        assert _rel(a, b) < 1e-3


@pytest.mark.parametrize("B,H,side,mr", CASES[:4])
def test_fused_attention_dropout_bf16_documented_tolerance(B, H, side, mr):
    qkv, tabs, go = _inputs(B, H, side, mr, seed=6)
    keep = _keep(77, 0.2, B, H, side * side + 1)
    ref_out, ref_g = _oracle_drop(qkv, tabs, go, mr, keep)
    out, g = _fused_drop(qkv, tabs, go, mr, torch.bfloat16, 0.2, 77)
    assert _rel(out, ref_out) < 2e-2
    for a, b in zip(g, ref_g):
        assert _rel(a, b) < 3e-2


def test_fused_attention_dropout_properties_at_full_size():
    """B = 128, H = 6, N = 197 in bf16: with V = 1 and zero value tables a row of the output is (kept count) / (1 - p) of
    softmax mass — its mean over everything is 1 within sampling noise and it is NOT constant; the same seed replays bit
    for bit (forward and backward), another seed gives another mask; p = 0 through the _drop entry points IS the plain path."""
    from cream_amd.autoformer import fused_attention as FA
    B, H, N, mr, p = 128, 6, 197, 14, 0.1
    g = torch.Generator(device=DEV).manual_seed(8)
    qkv = torch.randn(B, N, 3, H, 64, device=DEV, generator=g).bfloat16()
    tabs = [torch.randn(30, 64, device=DEV, generator=g) * 0.5 for _ in range(4)]
    zero = torch.zeros(30, 64, device=DEV)
    q1 = qkv.clone()
    q1[:, :, 2] = 1
    out = FA.attention_rpe2d_fused(q1, tabs[0], tabs[1], zero, zero, 0.125, mr, dropout_p=p, seed=3).float()
    assert abs(float(out.mean()) - 1.0) < 5e-3 and float(out.std()) > 1e-2
    res = []
    for seed in (11, 11, 12):
        x = [qkv.clone().requires_grad_()] + [t.clone().requires_grad_() for t in tabs]
        o = FA.attention_rpe2d_fused(x[0], *x[1:], 0.125, mr, dropout_p=p, seed=seed)
        o.backward(torch.ones_like(o))
        res.append([o.detach()] + [t.grad for t in x])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0], res[2][0])
    plain = FA.attention_rpe2d_fused(qkv, *tabs, 0.125, mr)
    assert torch.equal(FA.attention_rpe2d_fused(qkv, *tabs, 0.125, mr, dropout_p=0.0, seed=5), plain)


def test_attention_super_with_attn_drop_takes_the_fused_kernels():
    """AttentionSuper(attn_drop = 0.1) in training mode: 'auto' now resolves to the fused kernels (the run is replayed by
    torch.manual_seed), eval mode is the undropped path."""
    from cream_amd.autoformer import fused_attention as FA
    from cream_amd.autoformer.modules import AttentionSuper
    torch.manual_seed(0)
    m = AttentionSuper(384, num_heads=6, qkv_bias=True, attn_drop=0.1, relative_position=True, change_qkv=True,
                       max_relative_position=14).to(DEV)
    m.set_sample_config(sample_q_embed_dim=384, sample_num_heads=6, sample_in_embed_dim=384)
    x = torch.randn(2, 197, 384, device=DEV)
    calls = []
    orig = FA.attention_rpe2d_fused
    FA.attention_rpe2d_fused = lambda *a, **k: (calls.append(k.get("dropout_p")), orig(*a, **k))[1]
    try:
        m.train()
        torch.manual_seed(1); y1 = m(x)
        torch.manual_seed(1); y2 = m(x)
        torch.manual_seed(2); y3 = m(x)
        m.eval()
        y4 = m(x)
    finally:
        FA.attention_rpe2d_fused = orig
    assert calls == [0.1, 0.1, 0.1, 0.0]
    assert torch.equal(y1, y2) and not torch.equal(y1, y3) and not torch.equal(y1, y4)


def test_c_abi_dropout_rejects_bad_rates():
    import ctypes
    from cream_amd import _lib
    lib = _lib.load()
    q = torch.zeros(1, 5, 3, 1, 64, device=DEV)
    out = torch.zeros(1, 5, 1, 64, device=DEV)
    lse = torch.zeros(1, 1, 5, device=DEV)
    sp = torch.zeros(1, 1, 64, 32, device=DEV)
    t = torch.zeros(30, 64, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    args = lambda rate: (p(out), p(lse), p(sp), p(q), p(q), p(q), 960, 192, 64, p(t), p(t), p(t), p(t), 64, None,
                         1, 1, 5, 2, 2, 14, 0.125, rate, 7, _lib.F32, None)
    assert lib.cream_attn_rpe2d_fwd_drop(*args(0.25)) == 0
    assert lib.cream_attn_rpe2d_fwd_drop(*args(1.0)) == -1
    assert lib.cream_attn_rpe2d_fwd_drop(*args(-0.1)) == -1
    assert lib.cream_attn_rpe2d_fwd_drop(*args(float("nan"))) == -1
    torch.cuda.synchronize()


# ---- persistent grids smaller than the problem (cream_cu_reserve, the data-parallel driver's CU reserve) ----------------------------
# (B, H, side, max_rel): more (b, h) items than the 8 workgroups of an 8-CU budget, and no multiple of 8: uneven items per workgroup,
# the next item's operands travelling under the current item's work, the last item without a successor
SMALL_GRID = [(5, 2, 7, 14), (3, 3, 15, 14), (11, 1, 5, 3), (3, 3, 14, 14)]


class _CuBudget:
    """`with _CuBudget(8) as lib:` sizes every persistent grid for 8 CUs (None: all of them) and puts the reserve back."""

    def __init__(self, cus):
        self.cus = cus

    def __enter__(self):
        from cream_amd import _lib
        lib = _lib.load()
        self.lib, self.prev = lib, lib.cream_cu_reserve(0)
        if self.cus is not None:
            lib.cream_cu_reserve(lib.cream_cu_count() - self.cus)
            assert lib.cream_cu_count() == self.cus
        return lib

    def __exit__(self, *exc):
        self.lib.cream_cu_reserve(self.prev)


def _small_and_full_grid(run, B, H):
    """run() at the 8-CU budget twice and at the full budget -> (small, full); the rerun reproduces every bit, the table-gradient
    partials followed the budget (or the Python side sized them for the wrong grid), output and dqkv do not depend on which
    workgroup ran an item, the table gradients only through the order of the per-workgroup fp32 chains (1e-5)."""
    with _CuBudget(8) as lib:
        assert lib.cream_attn_rpe2d_dtab_parts(B, H) == 8 < B * H and (B * H) % 8 != 0
        small, again = run(), run()
    with _CuBudget(None) as lib:
        assert lib.cream_attn_rpe2d_dtab_parts(B, H) == B * H
        full = run()
    assert torch.equal(small[0], again[0]) and all(torch.equal(a, b) for a, b in zip(small[1], again[1]))
    assert torch.isfinite(small[0]).all() and all(torch.isfinite(t).all() for t in small[1])
    assert torch.equal(small[0], full[0]) and torch.equal(small[1][0], full[1][0])
    for a, b in zip(small[1][1:], full[1][1:]):
        assert _rel(a, b) < 1e-5
    return small, full


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,side,mr", SMALL_GRID)
def test_fused_attention_on_a_grid_smaller_than_the_items(B, H, side, mr, dtype):
    """Every instantiation (fp32, bf16; the AutoFormer geometry, the generic ones) with several items per workgroup:
    oracle parity at the documented tolerances, and the same bits as on the full grid."""
    qkv, tabs, go = _inputs(B, H, side, mr, seed=7)
    ref_out, ref_g = _oracle(qkv, tabs, go, mr)
    (out, g), _ = _small_and_full_grid(lambda: _fused(qkv, tabs, go, mr, dtype), B, H)
    assert _rel(out, ref_out) < (1e-3 if dtype == torch.float32 else 2e-2)
    for a, b in zip(g, ref_g):
        assert _rel(a, b) < (1e-3 if dtype == torch.float32 else 3e-2)


@pytest.mark.parametrize("fwd_mode", [0, 1])
@pytest.mark.parametrize("bwd_mode", [0, 1, 2])
def test_kernel_variants_of_the_benchmark_geometry_on_a_grid_smaller_than_the_items(bwd_mode, fwd_mode):
    """N = 197 in bf16: both forward kernels and the three backward implementations walk several items per workgroup."""
    from cream_amd import _lib
    lib = _lib.load()
    B, H, side, mr = 3, 3, 14, 14
    qkv, tabs, go = _inputs(B, H, side, mr, seed=8)
    ref_out, ref_g = _oracle(qkv, tabs, go, mr)
    prev_b, prev_f = lib.cream_attn_rpe2d_bwd_mode(-1), lib.cream_attn_rpe2d_fwd_mode(-1)
    try:
        lib.cream_attn_rpe2d_bwd_mode(bwd_mode)
        lib.cream_attn_rpe2d_fwd_mode(fwd_mode)
        (out, g), _ = _small_and_full_grid(lambda: _fused(qkv, tabs, go, mr, torch.bfloat16), B, H)
    finally:
        lib.cream_attn_rpe2d_bwd_mode(prev_b)
        lib.cream_attn_rpe2d_fwd_mode(prev_f)
    assert _rel(out, ref_out) < 2e-2
    for a, b in zip(g, ref_g):
        assert _rel(a, b) < 3e-2


def test_fused_attention_dropout_on_a_grid_smaller_than_the_items():
    B, H, side, mr, p, seed = 5, 2, 7, 14, 0.1, 4321
    qkv, tabs, go = _inputs(B, H, side, mr, seed=9)
    ref_out, ref_g = _oracle_drop(qkv, tabs, go, mr, _keep(seed, p, B, H, side * side + 1))
    (out, g), _ = _small_and_full_grid(lambda: _fused_drop(qkv, tabs, go, mr, torch.float32, p, seed), B, H)
    assert _rel(out, ref_out) < 1e-3
    for a, b in zip(g, ref_g):
        assert _rel(a, b) < 1e-3
