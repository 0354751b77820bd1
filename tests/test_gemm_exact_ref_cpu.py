"""The exactness conditions of tests/gemm_exact_ref.py, proven by the fp64 references alone (no GPU): every case of the shared
list, with the seed the GPU tests use, keeps every result within the cap under which bf16 holds it exactly — the references
assert that themselves — and the operands are what the module says they are (ternary x a power of two, NaN outside the
active block)."""
import pytest
import torch

import gemm_exact_ref as R

CASES = R.all_cases()


def test_case_list_covers_what_it_claims():
    ks = {c for fam, c in R.TAIL_CASES if fam == "128x64"}
    assert {k % 64 for k in ks if k > 128} == {8, 16, 24, 32, 40, 48, 56} and {8, 24, 56, 64, 72, 120, 128} <= ks
    assert {c % 64 for fam, c in R.TAIL_CASES if fam == "256x256-longK"} == {0, 8, 16, 24, 32, 40, 48, 56}
    assert all(c >= 1152 for fam, c in R.TAIL_CASES if fam == "256x256-longK")
    assert max(c.M for c in CASES) == 1032 and max(c.M * c.N * c.K for c in CASES) <= 1032 * 2496 * 624
    assert all(c.N % 8 == 0 and c.K % 8 == 0 for c in CASES)
    # supernet-B: K % 64 in {16, 48} directly, the hidden widths' tails inside the 256-wide tile, the column edges, qkv widths
    assert {c.K % 64 for c in R.SPACE_B if c.seg} == {16, 0, 48}
    assert {c.K % 64 for c in R.SPACE_B if c.K >= 1584} == {48, 56, 0, 32, 16, 8}
    assert {c.N % 256 for c in R.SPACE_B if c.N in (528, 576, 624)} == {16, 64, 112}
    assert {1728, 1920} <= {c.N for c in R.SPACE_B if c.seg}
    assert any(c.nvalid == 756 for c in R.SPACE_T) and any(c.xzero == 756 for c in R.SPACE_T)
    # small grids: at least 2.5 x as many tiles as workgroups at 8 CUs, not divisible (the 256 x 192 tile cannot: see the list)
    for fam, a, _ in R.GRID_CASES:
        bm, bn, wgs = {"128x64": (128, 64, 24), "128x128": (128, 128, 16), "256x192-N384": (256, 192, 8)}.get(fam, (256, 256, 8))
        tiles = -(-a.M // bm) * -(-a.N // bn)
        assert tiles % wgs != 0 and (tiles >= 2.5 * wgs or fam.startswith("256x192")), (fam, tiles)


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_every_reference_is_exact_in_bf16(case):
    c = case
    o = R.operands(c, 0)
    # operands: ternary x a power of two, poisoned outside the active block
    for t, s in ((o.X, R.SX), (o.DY, R.SDY), (o.W, R.SW)):
        assert set((t / s).unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert o.ldw > c.K and o.ldw % 8 == 0 and o.wsup.shape == (c.N + 64, o.ldw) and o.wt.shape == (o.ldw, c.N + 64)
    assert o.wsup[c.N:].isnan().all() and o.wsup[:, c.K:].isnan().all() and o.wt[c.K:].isnan().all() and o.wt[:, c.N:].isnan().all()
    for buf in (o.x, o.dy, o.factor):
        assert buf[c.M:].isnan().all() and buf.shape[0] == c.M + R.PAD_ROWS and not buf[:c.M].isnan().any()
    assert float(o.F.min()) > 0 and float(o.F.max()) <= 1.13
    assert o.bias[c.N:].isnan().all() and o.bias_gelu[c.N:].isnan().all()
    assert float((o.bias_gelu[:c.N].double() * 16).abs().max()) <= 32
    if c.xzero:
        assert float(o.X[:, c.xzero:].abs().max()) == 0.0
    # every reference once: each asserts its cap and that the bf16 rounding is the identity
    out = R.ref_fwd(o)
    assert out.dtype == torch.bfloat16 and torch.equal(out.double(), o.X @ o.W.t() + o.bias[:c.N].double())
    R.ref_fwd(o, bias=False)
    dx = R.ref_dgrad(o)
    assert torch.equal(dx.double(), o.DY @ o.W)
    dh, prod = R.ref_dgrad_mul(o)
    assert bool(((dh.double() - prod).abs() <= 2.0 ** -8 * prod.abs()).all())          # ONE rounding (8-bit significand) of an exact product
    h, g, gp = R.ref_gelu(o)
    assert float(h.double().abs().max()) <= 16.0 and torch.isfinite(g).all() and torch.isfinite(gp).all()
    if c.nvalid:
        assert float(g[:, c.nvalid:].abs().max()) == 0.0 and float(gp[:, c.nvalid:].abs().max()) == 0.0
    if c.seg:
        assert o.w3.shape == (3, c.seg + 64, o.ldw) and o.w3[:, c.seg:].isnan().all() and o.w3[:, :, c.K:].isnan().all()
        assert torch.equal(o.wt3.float().nan_to_num(7.0), o.w3.transpose(1, 2).float().nan_to_num(7.0))     # poisoned the same way
        R.ref_fwd_seg(o)
        R.ref_dgrad_seg(o)
    w = R.ref_wgrad(o)
    assert R.wgrad_cap_for_every_split(o) <= R.CAP                 # every slice of whole 64-row steps, whatever S a device picks
    for S in {1, min(3, (c.M + 63) // 64), (c.M + 63) // 64}:
        parts = R.ref_wgrad_parts(o, S)
        assert torch.equal(parts.double().sum(0), w)
        sl = R.wgrad_slices(c.M, S)
        assert sl[0][0] == 0 and sl[-1][1] == c.M and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
    assert torch.equal(R.ref_colsum_dy(o), o.dy[:c.M].double().sum(0))
