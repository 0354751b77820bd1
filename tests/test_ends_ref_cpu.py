"""CPU checks of tests/ends_ref.py: the float64 references that tests/test_ends_gpu.py holds the stem, tail, loss and
AdamW kernels to are themselves pinned here against float64 runs of the framework's operators (F.layer_norm and its
autograd, F.unfold, log_softmax and its autograd, torch.optim.AdamW), so that a wrong reference cannot pass a wrong
kernel.  float64 against float64: the two sides differ only in the order of a few operations."""
import pytest
import torch
import torch.nn.functional as F

import ends_ref as R

TIGHT = dict(rtol=1e-12, atol=1e-13)


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("B,C,H,W,ph,pw", [(2, 3, 32, 32, 16, 16), (1, 1, 8, 24, 8, 8), (3, 2, 48, 16, 16, 8), (1, 3, 24, 48, 8, 24)])
def test_unfold_is_f_unfold_in_c_i_j_order(B, C, H, W, ph, pw):
    img = _rand(B, C, H, W)
    want = F.unfold(img, kernel_size=(ph, pw), stride=(ph, pw)).transpose(1, 2).reshape(-1, C * ph * pw)
    assert torch.equal(R.unfold(img, ph, pw), want)
    # element (c, i, j) of patch (b, gi, gj), spelled out once
    b, gi, gj, c, i, j = B - 1, H // ph - 1, W // pw - 1, C - 1, ph - 2, pw - 3
    row = (b * (H // ph) + gi) * (W // pw) + gj
    assert R.unfold(img, ph, pw)[row, (c * ph + i) * pw + j] == img[b, c, gi * ph + i, gj * pw + j]


@pytest.mark.parametrize("with_pos", [False, True])
def test_stem_assemble_and_backward_are_cat_plus_pos_and_its_autograd(with_pos):
    B, N, E = 19, 5, 12
    y, cls, pos = _rand(B, N - 1, E, seed=1), _rand(E, seed=2), (_rand(N, E, seed=3) if with_pos else None)
    yr, cr = y.clone().requires_grad_(), cls.clone().requires_grad_()
    pr = pos.clone().requires_grad_() if with_pos else None
    x0 = torch.cat([cr.expand(B, 1, E), yr], dim=1)
    if with_pos:
        x0 = x0 + pr
    assert torch.equal(R.stem_assemble(y, cls, pos), x0.detach())
    dx0 = _rand(B, N, E, seed=4)
    x0.backward(dx0)
    dy, psum = R.stem_bwd(dx0)
    assert torch.equal(dy, yr.grad)
    assert psum.shape == (2, N, E)                                      # 16 images + a ragged chunk of 3
    assert torch.equal(psum[0], dx0[:16].sum(0)) and torch.equal(psum[1], dx0[16:].sum(0))
    torch.testing.assert_close(psum.sum(0)[0], cr.grad, **TIGHT)        # class-token gradient
    if with_pos:
        torch.testing.assert_close(psum.sum(0), pr.grad, **TIGHT)       # position-embedding gradient


@pytest.mark.parametrize("variant", ["no_f", "f_scaled", "f_unscaled"])
def test_tail_reference_is_layer_norm_then_token_mean(variant):
    B, N, E, eps = 3, 7, 20, 1e-6
    x1, gamma, beta, g = _rand(B, N, E, seed=5) * 2 + 0.5, _rand(E, seed=6), _rand(E, seed=7), _rand(B, E, seed=8)
    f = _rand(B, N, E, seed=9) if variant != "no_f" else None
    s = torch.tensor([0.0, 1.25, 0.5], dtype=torch.float64) if variant == "f_scaled" else None
    x = x1 if f is None else x1 + (s[:, None, None] if s is not None else 1.0) * f
    xr = x.clone().requires_grad_()
    pooled_f = F.layer_norm(xr, (E,), gamma, beta, eps)[:, 1:].mean(1)
    pooled, xm, mean, rstd = R.tail_fwd(x1, f, s, gamma, beta, eps)
    torch.testing.assert_close(pooled, pooled_f.detach(), **TIGHT)
    torch.testing.assert_close(xm, F.layer_norm(x, (E,), None, None, eps)[:, 1:].mean(1), **TIGHT)
    torch.testing.assert_close(mean, x.mean(-1), **TIGHT)
    torch.testing.assert_close(rstd, (x.var(-1, unbiased=False) + eps).rsqrt(), **TIGHT)
    pooled_f.backward(g)
    dx, dxs = R.tail_bwd(g, x1, f, s, gamma, beta, eps)
    torch.testing.assert_close(dx, xr.grad, **TIGHT)
    assert float(dx[:, 0].abs().max()) == 0.0                           # the class token does not reach the output
    torch.testing.assert_close(dxs, xr.grad * (s[:, None, None] if s is not None else 1.0), **TIGHT)
    # the sample scale counts only together with f
    if f is None:
        again = R.tail_fwd(x1, None, torch.tensor([3.0, 0.0, 1.0], dtype=torch.float64), gamma, beta, eps)
        assert torch.equal(again[0], pooled)


def test_tail_reference_keeps_the_variance_of_a_large_offset():
    """x = 100 + 0.01 randn: E[x^2] - E[x]^2 in fp32 would lose rstd; the reference subtracts the mean first."""
    x1 = 100 + 0.01 * _rand(2, 3, 256, seed=10)
    _, _, mean, rstd = R.tail_fwd(x1.float(), None, None, torch.ones(256), torch.zeros(256), 1e-6)
    xd = x1.float().double()
    torch.testing.assert_close(rstd, (xd.var(-1, unbiased=False) + 1e-6).rsqrt(), rtol=1e-9, atol=0)
    assert 50 < float(rstd.min()) < float(rstd.max()) < 200 and abs(float(mean.mean()) - 100) < 1e-2


@pytest.mark.parametrize("C", [1, 2, 37, 257])
@pytest.mark.parametrize("tsum", [1.0, 0.5, 2.0])
def test_soft_ce_reference_is_log_softmax_and_its_autograd(C, tsum):
    B, gs = 3, 1.0 / 3
    x = (_rand(B, C, seed=C) * 30).requires_grad_()
    t = torch.softmax(_rand(B, C, seed=C + 1), -1) * tsum
    rows = torch.sum(-t * torch.log_softmax(x, -1), -1)
    (gx,) = torch.autograd.grad(rows.sum() * gs, x)
    loss, dl = R.soft_ce(x.detach(), t, gs)
    torch.testing.assert_close(loss, rows.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dl, gx, rtol=1e-12, atol=1e-15)


def test_soft_ce_reference_ignores_minus_inf_at_a_zero_target():
    B, C = 3, 9
    x, t = _rand(B, C, seed=11) * 80, torch.softmax(_rand(B, C, seed=12), -1)
    t[:, 4] = 0.0
    xi = x.clone()
    xi[:, 4] = float("-inf")
    keep = [c for c in range(C) if c != 4]
    loss, dl = R.soft_ce(xi, t, 1.0)
    loss_k, dl_k = R.soft_ce(x[:, keep], t[:, keep], 1.0)
    assert torch.isfinite(loss).all() and torch.isfinite(dl).all()
    torch.testing.assert_close(loss, loss_k, rtol=1e-13, atol=0)        # an exact zero more in the sums: another order
    torch.testing.assert_close(dl[:, keep], dl_k, rtol=1e-12, atol=1e-15)
    assert float(dl[:, 4].abs().max()) == 0.0
    # one-hot targets: the loss is the negative log-probability of the class
    hot = F.one_hot(torch.tensor([0, 8, 3]), C).double()
    torch.testing.assert_close(R.soft_ce(x, hot, 1.0)[0], F.cross_entropy(x, torch.tensor([0, 8, 3]), reduction="none"),
                               rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_adamw_reference_is_torch_optim_adamw(wd):
    lr, b1, b2, eps = 3e-3, 0.9, 0.999, 1e-8
    p0 = _rand(23, 7, seed=13)
    grads = [_rand(23, 7, seed=20 + k) * (10.0 ** (k - 1)) for k in range(4)]
    for g in grads:
        g[1::7] = 1e-12
        g[::5] = 0.0                                                    # v stays 0 there: eps decides
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for k, g in enumerate(grads):
        q.grad = g.clone()
        opt.step()
        p, m, v = R.adamw_step(p, g, m, v, lr, b1, b2, eps, wd, k + 1)
        st = opt.state[q]
        torch.testing.assert_close(p, q.detach(), rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(m, st["exp_avg"], rtol=1e-13, atol=0)
        torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-13, atol=0)
    assert float(v[::5].abs().max()) == 0.0                             # 0 / (0 + eps): only the decay moves p there
    torch.testing.assert_close(p[::5], p0[::5] * (1 - lr * wd) ** 4, rtol=1e-14, atol=0)
    # a late step from given moments
    opt.state[q]["step"] = torch.tensor(999.0) if torch.is_tensor(opt.state[q]["step"]) else 999
    q.grad = grads[1].clone()
    opt.step()
    p, m, v = R.adamw_step(p, grads[1], m, v, lr, b1, b2, eps, wd, 1000)
    torch.testing.assert_close(p, q.detach(), rtol=1e-13, atol=1e-15)


def test_deinterleave_sends_super_row_3i_plus_j_to_part_j_row_i():
    w = _rand(12, 5, seed=14)
    d = R.deinterleave(w)
    assert d.shape == (3, 4, 5)
    for i in range(4):
        for j in range(3):
            assert torch.equal(d[j, i], w[3 * i + j])
    assert torch.equal(d, torch.stack([w[j::3] for j in range(3)]))


def test_tolerance_rule_accepts_a_reordered_sum_and_refuses_a_dropped_term():
    """The rule of check_against_fp32_baseline on a plain fp32 row sum: another summation order passes, a sum that
    leaves one of E = 1280 terms out (an error of about 1 / E) does not, and neither does a non-finite result."""
    x = (_rand(64, 1280, seed=15) * 0.5 + 2).float()
    ref = x.double().sum(-1)
    base = x.sum(-1)
    other = x.view(64, 4, 320).sum(-1).sum(-1)                          # four partial sums, then their sum
    ok, u_k, u_fw = R.check_against_fp32_baseline(other, base, ref)
    assert ok and u_k < 64 and u_fw < 64
    dropped = x[:, 1:].sum(-1)
    assert not R.check_against_fp32_baseline(dropped, base, ref)[0]
    bad = other.clone()
    bad[3] = float("nan")
    assert not R.check_against_fp32_baseline(bad, base, ref)[0]
    # the floor: 4 ulp of the row's largest value and nothing more
    r = torch.tensor([[1.0, 1e-6]], dtype=torch.float64)
    assert R.check_against_fp32_baseline(r + 4 * R.ULP32, r, r)[0] and not R.check_against_fp32_baseline(r + 5 * R.ULP32, r, r)[0]
    assert not R.check_against_fp32_baseline(r * (1 + 5 * R.ULP32), r, r, floor="elem")[0]
    assert R.check_against_fp32_baseline(r * (1 + 3 * R.ULP32), r, r, floor="elem")[0]
    # a baseline that is 2 ulp (of the row / of the element) off buys the kernel 4 x 2 + 4 ulp
    assert R.check_against_fp32_baseline(r + 12 * R.ULP32, r + 2 * R.ULP32, r)[0]
    assert not R.check_against_fp32_baseline(r + 13 * R.ULP32, r + 2 * R.ULP32, r)[0]
    assert R.check_against_fp32_baseline(r * (1 + 11 * R.ULP32), r * (1 + 2 * R.ULP32), r, floor="elem")[0]
    assert not R.check_against_fp32_baseline(r * (1 + 13 * R.ULP32), r * (1 + 2 * R.ULP32), r, floor="elem")[0]
    # an exact zero of the reference that the baseline reproduces must be reproduced by the kernel
    z = torch.tensor([[0.0, 0.0]], dtype=torch.float64)
    assert R.check_against_fp32_baseline(z, z, z)[0] and not R.check_against_fp32_baseline(z + 1e-30, z, z)[0]
