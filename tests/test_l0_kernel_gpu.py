"""The kernels of cream_amd/csrc/l0_mask.hip on the device against the fp64 references and derived bounds of tests/l0_ref.py:
masked LayerNorm (forward with / without the folded residual, backward with / without dres and dx_scaled), the masked
operand pack (bit-exact), the masked gradient finalisation (bounds, run-to-run and grid-independent bit-reproducibility)."""
import pytest
import torch

import l0_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN_ROWS = (1, 129, 4 * 1024 + 1)        # one row; more than one workgroup; one more row than a pass of the backward's 1024 x 4 waves


def _dev(t):
    return t.to(DEV) if t is not None else None


@pytest.mark.parametrize("E", [64, 128, 520])
@pytest.mark.parametrize("pattern", R.KEEP_PATTERNS)
def test_masked_layernorm(E, pattern):
    from cream_amd import _lib
    from cream_amd.tinyclip import mask_ops as K
    assert _lib.load().cream_ln_partials() == 1024
    for M in LN_ROWS:
        for with_res in (False, True):
            c = R.ln_case(M, E, pattern, with_res)
            hm = K.HiddenMask(_dev(c["z"]))
            g, b = _dev(c["gamma"]), _dev(c["beta"])
            if with_res:
                xsum, y, mean, rstd = K.add_ln_fwd_masked(_dev(c["x"]), _dev(c["res"]), _dev(c["scale"]), c["rows_per_sample"], g, b, c["eps"], hm)
            else:
                y, mean, rstd = K.ln_fwd_masked(_dev(c["x"]), g, b, c["eps"], hm)
                xsum = None
            worst = R.check_ln_fwd(dict(y=y, mean=mean, rstd=rstd, xsum=xsum), c)
            for with_dres, with_scaled in ((with_res, not with_res), (not with_res, not with_res)):
                bc = R.ln_bwd_case(c, with_dres, with_scaled)
                dx, dxs, part = K.ln_bwd_masked_raw(_dev(bc["dy"]), _dev(bc["xin"]), _dev(bc["mean"]), _dev(bc["rstd"]), g, hm,
                                                    _dev(bc["dres"]), _dev(bc["bscale"]), bc["rows_per_sample"], with_scaled)
                assert (dxs is not None) == with_scaled
                p64 = part.double().sum(0).cpu()
                wb = R.check_ln_bwd(dict(dx=dx, dxs=dxs, dgamma=p64[0], dbeta=p64[1], colsum=p64[2]), bc)
                assert bool((part[:, :2][:, :, _dev(c["z"]) == 0] == 0).all())                    # every slab partial, not only the sum
            print(f"[ln masked E={E} {pattern} M={M} res={with_res}] worst ratio to the bound: fwd {max(worst.values()):.2f}, bwd {max(wb.values()):.2f}")
    if pattern == "single_kept":                                       # n_keep = 1: the variance is 0 and y = beta in that column
        k = int(torch.where(c["z"] != 0)[0])
        assert torch.equal(y[:, k].cpu(), c["beta"][k].bfloat16().expand(y.shape[0]))


@pytest.mark.parametrize("shape", [(64, 64, 64), (72, 200, 1), (128, 512, 64), (128, 512, 1)])
def test_masked_pack_is_bit_exact(shape):
    from cream_amd.tinyclip import mask_ops as K
    rows, cols, cg = shape
    W = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols))
    r, c = R.mask_with_zeros(rows, 1), R.mask_with_zeros(cols // cg, 2)
    bias = torch.randn(cols, generator=torch.Generator().manual_seed(9))
    for rr, cc in ((r, None), (None, c), (r, c)):
        mir = torch.full((rows, cols), 7.0, dtype=torch.bfloat16, device=DEV)
        mir_t = torch.full((cols, rows), 7.0, dtype=torch.bfloat16, device=DEV)
        mb = torch.full((cols,), 7.0, dtype=torch.bfloat16, device=DEV)
        jobs = K.MaskPack()
        jobs.add(_dev(W), _dev(rr), _dev(cc), cg, mir=mir, mir_t=mir_t)
        if cc is not None and cg == 1:
            jobs.add(_dev(bias), None, _dev(cc), 1, mir=mb)             # a bias with its mask: rows = 1
        jobs.launch()
        want = R.pack_ref(W, rr, cc, cg)
        assert torch.equal(mir.cpu(), want), (shape, rr is not None, cc is not None)
        assert torch.equal(mir_t.cpu(), want.T)
        if cc is not None and cg == 1:
            assert torch.equal(mb.cpu(), (bias * cc).bfloat16())


def _run_finalize(f, overwrite, accumulate, with_r=True, with_c=True):
    from cream_amd.tinyclip import mask_ops as K
    dst, dr, dc = _dev(f["dst0"].clone()), _dev(f["dr0"].clone()), _dev(f["dc0"].clone())
    n, rows, cols = f["parts"].shape
    jobs = K.MaskGradJobs()
    jobs.add(dst, _dev(f["parts"]), n, rows * cols, _dev(f["W"]), _dev(f["r"]) if with_r else None, _dev(f["c"]) if with_c else None,
             f["c_group"], dr_out=dr, dc_out=dc, overwrite=overwrite, dr_accumulate=accumulate, dc_accumulate=accumulate)
    jobs.launch()
    torch.cuda.synchronize()
    return dict(dst=dst, dr=dr, dc=dc)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("nparts", [1, 3, 16])
@pytest.mark.parametrize("shape", [(128, 128, 64), (128, 520, 1)])
def test_masked_finalize(shape, nparts, bf16):
    from cream_amd import _lib
    rows, cols, cg = shape
    f = R.finalize_case(rows, cols, cg, nparts, bf16)
    lib = _lib.load()
    for overwrite, accumulate in ((False, False), (True, False), (False, True)):
        out = _run_finalize(f, overwrite, accumulate)
        worst = R.check_finalize(out, f, overwrite, accumulate)
        again = _run_finalize(f, overwrite, accumulate)
        assert all(torch.equal(out[k], again[k]) for k in out), "two runs differ"
        prev = lib.cream_cu_reserve(-1)
        try:
            got = []
            for reserve in (0, 10 ** 6):                               # every CU / one CU per XCD: grids of 8 x 256 and 8 x 8 workgroups at the most
                lib.cream_cu_reserve(reserve)
                got.append(_run_finalize(f, overwrite, accumulate))
        finally:
            lib.cream_cu_reserve(prev)
        assert all(torch.equal(got[0][k], got[1][k]) and torch.equal(got[0][k], out[k]) for k in out), "the grid changes the result"
    print(f"[mask finalize {shape} parts={nparts} bf16={bf16}] worst ratio to the bound {max(worst.values()):.2f}")


@pytest.mark.parametrize("nparts", [3, 16, 40, 100])
def test_masked_finalize_adds_the_parts_in_the_tree_of_grad_finalize(nparts):
    """Without masks dst is cream_grad_finalize's sum, bit for bit (4 / 16 / 64 part lanes)."""
    from cream_amd.autoformer import block as B
    f = R.finalize_case(128, 136, 1, nparts, False, seed=3)
    out = _run_finalize(f, True, False, with_r=False, with_c=False)
    p = torch.nn.Parameter(torch.zeros(128, 136, device=DEV))
    jobs = B.GradJobs()
    jobs.add(p, _dev(f["parts"]), nparts, 128 * 136, 128, 136)
    jobs.launch()
    torch.cuda.synchronize()
    assert torch.equal(p.grad, out["dst"])
