"""TinyCLIP's mask folding on the CPU (tests/l0_ref.py): the algebra against the composed masked mirror in fp64, and the
kernels' references — their fp32 models pass the derived bounds, every injected fault breaks one."""
import pytest
import torch

import l0_ref as R

LAYERS, WIDTH, HEADS = 2, 128, 2


def _tower(seed=0):
    from cream_amd.tinyclip.model import Transformer
    torch.manual_seed(seed)
    tr = Transformer(WIDTH, LAYERS, HEADS).double()
    with torch.no_grad():
        for n, p in tr.named_parameters():
            if n.endswith("bias") or "ln_" in n:
                p.add_(0.1 * torch.randn_like(p))
    return tr


def _masks(seed=1):
    g = torch.Generator().manual_seed(seed)
    zh = torch.rand(WIDTH, generator=g, dtype=torch.float64)
    zh[torch.rand(WIDTH, generator=g) < 0.3] = 0
    zd = torch.rand(LAYERS, HEADS, generator=g, dtype=torch.float64)
    zd[0, 1] = 0                                                        # a fully dropped head
    zi = torch.rand(LAYERS, 4 * WIDTH, generator=g, dtype=torch.float64)
    zi[torch.rand(LAYERS, 4 * WIDTH, generator=g) < 0.4] = 0
    return zh, zd, zi


@pytest.mark.parametrize("causal", [False, True])
def test_folding_identity_against_the_composed_masked_mirror(causal):
    """Forward, input gradient, every weight gradient and the three mask gradients.  Both sides are fp64 evaluations of the
    same real function in different operation orders: the difference is rounding, unit roundoff 2^-53 per operation over the
    longest chains (a dot product of 4 D terms, N L terms per weight-gradient entry, through `LAYERS` blocks) — 8 operations
    per term of slack, relative to the largest entry of the tensor compared."""
    N, L = 2, 5
    tr = _tower()
    zh, zd, zi = (z.clone().requires_grad_() for z in _masks())
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(N, L, WIDTH, generator=g, dtype=torch.float64) * (zh.detach() != 0)
    gy = torch.randn(N, L, WIDTH, generator=g, dtype=torch.float64)
    x = x0.clone().requires_grad_()
    mask = torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1) if causal else None
    y = tr(x, attn_mask=mask, causal=causal, hidden_z=zh, heads_z=zd, intermediate_z=zi)
    y.backward(gy)
    fy, fdx, fgrads, fdzh, fdzd, fdzi = R.folded_tower(tr.resblocks, x0, gy, zh.detach(), zd.detach(), zi.detach(), HEADS, causal)
    tol = LAYERS * (4 * WIDTH + 4 * WIDTH + N * L) * 8 * 2.0 ** -53

    def rel(a, b):
        return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-300))
    errs = {"y": rel(fy, y.detach()), "dx": rel(fdx, x.grad), "dzh": rel(fdzh, zh.grad), "dzd": rel(fdzd, zd.grad), "dzi": rel(fdzi, zi.grad)}
    for i, blk in enumerate(tr.resblocks):
        for k, p in blk.named_parameters():
            errs[f"{i}.{k}"] = rel(fgrads[i][k], p.grad)
    print(f"[l0 folding causal={causal}] worst {max(errs.values()):.1e} (bound {tol:.1e})")
    assert max(errs.values()) < tol, {k: v for k, v in errs.items() if v >= tol}
    assert bool((zd.grad[0, 1] != 0)) and bool((y.detach()[..., zh.detach() == 0] == 0).all())


LN_CASES = [(1, 64), (129, 128), (7, 520)]


@pytest.mark.parametrize("pattern", R.KEEP_PATTERNS)
@pytest.mark.parametrize("with_res", [False, True])
def test_masked_layernorm_model_meets_the_bounds(pattern, with_res):
    for M, E in LN_CASES:
        c = R.ln_case(M, E, pattern, with_res)
        R.check_ln_fwd(R.ln_fwd_model(c), c)
        b = R.ln_bwd_case(c, with_dres=with_res, with_scaled=not with_res)
        R.check_ln_bwd(R.ln_bwd_model(b), b)
    if pattern == "single_kept":
        c = R.ln_case(3, 64, pattern, False)
        y = R.ln_fwd_model(c)["y"]
        k = int(torch.where(c["z"] != 0)[0])
        assert torch.equal(y[:, k], c["beta"][k].bfloat16().expand(3))        # variance 0: y = beta


@pytest.mark.parametrize("fault", ["dropped_in_stats", "divisor_E"])
def test_masked_layernorm_bounds_catch_the_faults(fault):
    c = R.ln_case(129, 128, "every_second", True)
    with pytest.raises(AssertionError):
        R.check_ln_fwd(R.ln_fwd_model(c, fault), c)
    b = R.ln_bwd_case(c, True, True)
    with pytest.raises(AssertionError):
        R.check_ln_bwd(R.ln_bwd_model(b, fault), b)


def test_pack_reference_and_its_faults():
    W = torch.randn(128, 128, generator=torch.Generator().manual_seed(1))
    r, c = R.mask_with_zeros(128, 2), R.mask_with_zeros(128, 3)
    want = R.pack_ref(W, r, c, 1)
    assert torch.equal(want, ((W * r[:, None]) * c[None, :]).bfloat16())
    assert not torch.equal(R.pack_ref(W, r, c, 1, "rc_swapped"), want)
    ch = torch.tensor([0.0, 0.7])
    assert not torch.equal(R.pack_ref(W, r, ch, 64, "c_group_ignored"), R.pack_ref(W, r, ch, 64))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("nparts", [1, 3, 16])
def test_finalize_model_meets_the_bounds_and_faults_do_not(bf16, nparts):
    for rows, cols, cg in ((128, 128, 64), (128, 520, 1), (128, 128, 1)):
        f = R.finalize_case(rows, cols, cg, nparts, bf16)
        for overwrite in (False, True):
            R.check_finalize(R.finalize_model(f, overwrite), f, overwrite)
        R.check_finalize(R.finalize_model(f, False, True), f, False, True)
        faults = ["last_part_skipped"] + (["c_group_ignored"] if cg == 64 else []) + (["rc_swapped"] if rows == cols and cg == 1 else [])
        for fault in faults:
            with pytest.raises(AssertionError):
                R.check_finalize(R.finalize_model(f, True, fault=fault), f, True)


def test_entry_points_validate_their_arguments():
    """No device: the checks return error codes before anything is launched."""
    import ctypes
    from cream_amd import _lib
    lib = _lib.load()
    a = 0x1000
    assert lib.cream_ln_fwd_masked(a, a, a, a, a, a, a, 0, 4, 64, 1e-5, None) == -1             # n_keep = 0
    assert lib.cream_add_ln_fwd_masked(a, a, a, a, a, a, None, 1, a, a, a, 0, 4, 64, 1e-5, None) == -1
    assert lib.cream_ln_bwd_masked(a, None, a, a, a, a, a, a, a, 0, None, None, 1, 4, 64, None) == -1
    assert lib.cream_ln_fwd_masked(a, a, a, a, a, a, a, 65, 4, 64, 1e-5, None) == -1            # more kept columns than columns
    assert lib.cream_ln_fwd_masked(a, a, a, a, a, a, a, 3, 4, 66, 1e-5, None) == -4             # E % 4
    assert lib.cream_ln_fwd_masked(a, a, a, a, a, a, None, 3, 4, 64, 1e-5, None) == -1          # no mask
    assert lib.cream_ln_fwd_masked(None, None, None, None, None, None, None, 3, 0, 64, 1e-5, None) == 0
    pj = (_lib.MaskPackJob * 2)()
    pj[0].w, pj[0].mir, pj[0].ld, pj[0].ld_mir, pj[0].rows, pj[0].cols, pj[0].c_group = a, a, 64, 64, 64, 64, 1
    cast = lambda t: ctypes.cast(t, ctypes.c_void_p)                   # noqa: E731
    assert lib.cream_mask_pack_check(cast(pj), 1) == 0 and lib.cream_mask_pack_check(cast(pj), 0) == 0
    assert lib.cream_mask_pack_check(None, 1) == -1 and lib.cream_mask_pack_check(cast(pj), _lib.MAX_MASK_JOBS + 1) == -1
    pj[0].c_group = 32
    assert lib.cream_mask_pack_check(cast(pj), 1) == -1
    pj[0].c_group, pj[0].cols = 1, 66
    assert lib.cream_mask_pack_check(cast(pj), 1) == -1
    gj = (_lib.MaskGradJob * 2)()
    for j, base in ((gj[0], 0x10000), (gj[1], 0x20000)):
        j.dst, j.src, j.w, j.dr_out, j.ws = base, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000
        j.ld, j.pstride, j.ld_w, j.nparts, j.rows, j.cols, j.c_group = 64, 4096, 64, 2, 64, 64, 1
    assert lib.cream_mask_grad_check(cast(gj), 2) == 0
    assert lib.cream_mask_grad_ws_floats(128, 520) == 9 * 128 + 8 * 520 and lib.cream_mask_grad_ws_floats(0, 4) == 0
    gj[1].dr_out = gj[0].dr_out                                         # two writers of one output
    assert lib.cream_mask_grad_check(cast(gj), 2) == -1
    gj[1].dr_out, gj[1].ws = 0x23000, None                              # a mask gradient without its workspace
    assert lib.cream_mask_grad_check(cast(gj), 2) == -1
