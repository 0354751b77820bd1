"""Kernel-level parity of the two ends of the training step against the float64 references of tests/ends_ref.py:
csrc/stem_tail.hip (im2patch, stem assemble / backward, tail forward / backward, soft-target cross entropy) and
csrc/optim.hip (the one-launch AdamW with its bf16 operand copies), called through the C ABI on tiny tensors.

Rules of this file:
  * a pure cast or ONE fp32 operation is held to torch.equal;
  * fp32 sums and transcendental functions are held to ends_ref.check_against_fp32_baseline: the framework evaluates the
    same formula in fp32 on the same inputs, its elementwise error against float64 is measured, and the kernel may at no
    element be more than 4 x as far off, plus a floor of 4 fp32 ulp (error and floor taken per row on the scale of the
    row's largest reference value for sums, relative to the value itself for element-wise formulas such as the
    optimizer) — the margin covers another legitimate summation order, not a dropped element (>= 1 / E ~ 1e-3);
  * every output has a sentinel band behind it (and sentinels in its padding) that must survive, outputs are prefilled
    with NaN and must come back finite wherever the contract says they are written, readable padding the kernel must not
    use holds NaN.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import ends_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -1984.0                      # exact in bf16 and fp32
BAND = 64
OK, BAD_ARG, BAD_DTYPE, TOO_LARGE = 0, -1, -2, -4
NAN = float("nan")


def _lib():
    from cream_amd import _lib as L
    return L.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


class Guarded:
    """A buffer of `shape` (prefilled with `fill`) with BAND sentinel elements behind it; .t is the 16-byte aligned view."""

    def __init__(self, shape, dtype=torch.float32, fill=NAN):
        self.n = math.prod(shape)
        self.whole = torch.full((self.n + BAND,), SENT, dtype=dtype, device=DEV)
        self.t = self.whole[:self.n].view(shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.whole[self.n:] == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _hold(what, kernel, baseline, ref, floor="row", worst=None):
    ok, uk, uf = R.check_against_fp32_baseline(kernel, baseline, ref, floor)
    if worst is not None:
        w = worst.setdefault(what.split(" @")[0], [0.0, 0.0])
        w[0], w[1] = max(w[0], uk), max(w[1], uf)
    else:
        print(f"\n[ends] {what}: kernel {uk:.2f} ulp, framework fp32 {uf:.2f} ulp", end="")
    assert ok, f"{what}: kernel error {uk:.2f} ulp of the floor's scale against framework fp32 {uf:.2f} ulp"


def _report(tag, worst):
    for k, (uk, uf) in worst.items():
        print(f"\n[ends] {tag} {k}: worst kernel {uk:.2f} ulp, worst framework fp32 {uf:.2f} ulp", end="")


# ---- tail ---------------------------------------------------------------------------------------------------------------
# every E (template instantiations MAXC = 2 | 3 | 5 at both sides of 512 and 768, partly filled lane groups) with two N,
# every N (smallest; one 32-row chunk exactly; a one-row and a two-row last chunk; three chunks) with three E
TAIL_CASES = [
    (4, 2, 1, "no_f"), (4, 33, 3, "f_scaled"),
    (252, 5, 3, "f_scaled"), (252, 34, 1, "f_unscaled"),
    (256, 32, 3, "f_unscaled"), (256, 65, 3, "no_f_scale_given"),
    (260, 33, 1, "no_f"), (260, 2, 3, "f_scaled"),
    (512, 34, 3, "f_scaled"), (512, 5, 1, "f_unscaled"),
    (516, 65, 1, "f_unscaled"), (516, 32, 3, "no_f"),
    (768, 2, 3, "no_f_scale_given"), (768, 33, 3, "f_scaled"),
    (772, 5, 3, "f_scaled"), (772, 34, 3, "f_unscaled"),
    (1280, 32, 1, "f_unscaled"), (1280, 65, 3, "f_scaled"),
    (256, 5, 3, "large_offset"), (772, 33, 1, "large_offset"),
]


def _tail_inputs(E, N, B, variant):
    g = _gen(1000 * E + 10 * N + B)
    if variant == "large_offset":
        x1 = 100 + 0.01 * torch.randn(B, N, E, device=DEV, generator=g)     # a one-pass variance would lose rstd here
    else:
        x1 = torch.randn(B, N, E, device=DEV, generator=g) * 2 + 0.5
    f = scale = None
    if variant in ("f_scaled", "f_unscaled"):
        f = torch.randn(B, N, E, device=DEV, generator=g).bfloat16()
    if variant in ("f_scaled", "no_f_scale_given"):
        scale = torch.tensor([1.25, 0.0, 0.75][:B], device=DEV)
    gamma = torch.randn(E, device=DEV, generator=g) * 0.5 + 1.5
    beta = torch.randn(E, device=DEV, generator=g)
    gout = torch.randn(B, E, device=DEV, generator=g)
    return x1, f, scale, gamma, beta, gout


@pytest.mark.parametrize("E,N,B,variant", TAIL_CASES)
def test_tail_forward_and_backward_against_float64(E, N, B, variant):
    """cream_tail_fwd / cream_tail_bwd: pooled, xm, mean, rstd against the float64 LayerNorm + token mean, dx against its
    float64 autograd, dx_scaled == bf16(dx * s_b) bit for bit from the kernel's own dx, the class-token rows exactly zero,
    partial (cream_ln_partials() rows, those of workgroups without rows exactly zero) against the column sums of dx_scaled.
    'no_f_scale_given' pins the header's decision: without f the forward ignores sample_scale, the backward still applies it
    to dx_scaled.  'large_offset' is x1 = 100 + 0.01 randn.
    Measured on the MI355X (largest error in ulp of the floor's scale, worst over the cases; kernel / framework fp32):
    mean 0.30 / 0.30, rstd 1.17 / 1.73, xm 2.37 / 2.67, pooled 1.41 / 1.00, dx 4.69 / 4.56 (E = 4), partial 0.00 / 0.23;
    large_offset: mean 0.62 / 1.29, rstd 2.25 / 788 (the framework's fp32 variance is the worse one), xm 1566 / 3874,
    pooled 1546 / 3981, dx 317 / 436 (the mean's last bits are a large part of a row that varies by 0.01 around 100)."""
    lib, eps = _lib(), 1e-6
    x1, f, scale, gamma, beta, gout = _tail_inputs(E, N, B, variant)
    chunks, P = lib.cream_tail_chunks(N), lib.cream_ln_partials()
    assert chunks == -(-N // 32)
    pooled, xm, part = Guarded((B, E)), Guarded((B, E)), Guarded((B, chunks, E))
    mean, rstd = Guarded((B, N)), Guarded((B, N))
    rc = lib.cream_tail_fwd(_p(pooled.t), _p(xm.t), _p(part.t), _p(mean.t), _p(rstd.t), _p(x1), _p(f), _p(scale), _p(gamma),
                            _p(beta), B, N, E, eps, _stream())
    assert rc == OK
    torch.cuda.synchronize()
    for name, b in dict(pooled=pooled, xm=xm, part=part, mean=mean, rstd=rstd).items():
        assert b.intact(), f"{name}: sentinel band overwritten"
        assert bool(torch.isfinite(b.t).all()), f"{name}: not every element written"
    fwd_scale = scale if f is not None else None                          # the forward ignores the scale without f
    r_pooled, r_xm, r_mean, r_rstd = R.tail_fwd(x1, f, fwd_scale, gamma, beta, eps)
    x32 = x1 if f is None else x1 + (fwd_scale[:, None, None] if fwd_scale is not None else 1.0) * f.float()
    rowtop = x32.double().abs().amax(-1)
    tag = f"@ E={E} N={N} B={B} {variant}"
    _hold(f"tail mean {tag}", mean.t, x32.mean(-1), r_mean, floor=4 * R.ULP32 * rowtop)
    _hold(f"tail rstd {tag}", rstd.t, (x32.var(-1, unbiased=False) + eps).rsqrt(), r_rstd, floor="elem")
    fw_xm = F.layer_norm(x32, (E,), None, None, eps)[:, 1:].mean(1)
    _hold(f"tail xm {tag}", xm.t, fw_xm, r_xm)
    _hold(f"tail pooled {tag}", pooled.t, fw_xm * gamma + beta, r_pooled)

    # ---- backward, from the kernel's own mean / rstd --------------------------------------------------------------
    dx, dxs, partial = Guarded((B, N, E)), Guarded((B, N, E), torch.bfloat16), Guarded((P, E))
    rc = lib.cream_tail_bwd(_p(dx.t), _p(dxs.t), _p(partial.t), _p(gout), _p(x1), _p(f), _p(mean.t), _p(rstd.t), _p(gamma),
                            _p(scale), B, N, E, _stream())
    assert rc == OK
    torch.cuda.synchronize()
    for name, b in dict(dx=dx, dx_scaled=dxs, partial=partial).items():
        assert b.intact(), f"{name}: sentinel band overwritten"
        assert bool(torch.isfinite(b.t).all()), f"{name}: not every element written"
    assert partial.t.shape[0] == P
    r_dx, _ = R.tail_bwd(gout, x1, f, fwd_scale, gamma, beta, eps)
    xr = x32.clone().requires_grad_()
    (F.layer_norm(xr, (E,), gamma, beta, eps)[:, 1:].mean(1)).backward(gout)
    _hold(f"tail dx {tag}", dx.t, xr.grad, r_dx)
    assert float(dx.t[:, 0].abs().max()) == 0.0 and float(dxs.t[:, 0].float().abs().max()) == 0.0
    want = dx.t if scale is None else dx.t * scale[:, None, None]
    assert torch.equal(_bits(dxs.t), _bits(want.bfloat16())), "dx_scaled != bf16(dx * s_b)"
    M = B * N
    busy = min(P, -(-M // 4))                                             # workgroup p walks rows 4 p + wave, then + 4 P
    assert float(partial.t[busy:].abs().max() if busy < P else 0.0) == 0.0, "partial rows of idle workgroups are not zero"
    col = dxs.t.reshape(M, E)
    _hold(f"tail partial {tag}", partial.t.double().sum(0), col.float().sum(0), col.double().sum(0))


def test_tail_refuses_unsupported_shapes_without_launching():
    lib = _lib()
    buf = torch.zeros(4096, device=DEV)
    a = _p(buf)
    for E, N, want in [(1284, 2, TOO_LARGE), (6, 2, TOO_LARGE), (8, 1, BAD_ARG)]:
        assert lib.cream_tail_fwd(a, a, a, a, a, a, None, None, a, a, 1, N, E, 1e-6, _stream()) == want
        assert lib.cream_tail_bwd(a, a, a, a, a, None, a, a, a, None, 1, N, E, _stream()) == want
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


# ---- stem ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,ph,pw", [(2, 3, 32, 32, 16, 16), (1, 1, 8, 24, 8, 8), (3, 2, 48, 16, 16, 8), (1, 3, 24, 48, 8, 24)])
def test_im2patch_is_unfold_rounded_to_nearest_even(B, C, H, W, ph, pw):
    """cream_im2patch == bf16(F.unfold) in (c, i, j) order, bit for bit: non-square grids, ph != pw, a one-row grid, pw = 24;
    the image holds exact rounding ties of both parities, +-inf and fp32 denormals next to ordinary values."""
    lib = _lib()
    img = torch.randn(B, C, H, W, device=DEV, generator=_gen(H * W + pw))
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20,
                            float("inf"), float("-inf"), 1e-40, -1e-40, 2.0 ** -133, 3 * 2.0 ** -134, 0.0, 3.3895e38], device=DEV)
    flat = img.view(-1)
    pos = torch.arange(special.numel(), device=DEV) * 5 + 1
    flat[pos] = special
    flat[-special.numel():] = special
    out = Guarded((B * (H // ph) * (W // pw), C * ph * pw), torch.bfloat16)
    assert lib.cream_im2patch(_p(out.t), _p(img), B, C, H, W, ph, pw, _stream()) == OK
    torch.cuda.synchronize()
    assert out.intact()
    want = R.unfold(img.cpu(), ph, pw).bfloat16()                           # the CPU's cast: round to nearest even
    assert torch.equal(want, F.unfold(img.cpu(), (ph, pw), stride=(ph, pw)).transpose(1, 2).reshape(want.shape).bfloat16())
    assert torch.equal(_bits(out.t.cpu()), _bits(want))


def test_im2patch_refuses_an_unaligned_patch_width():
    lib = _lib()
    img = torch.zeros(1, 1, 8, 8, device=DEV)
    out = torch.zeros(4, 32, device=DEV, dtype=torch.bfloat16)
    assert lib.cream_im2patch(_p(out), _p(img), 1, 1, 8, 8, 8, 4, _stream()) == BAD_ARG


@pytest.mark.parametrize("E", [4, 36, 384])
def test_stem_assemble_is_one_exact_add(E):
    """cream_stem_assemble: x0 = cat(cls, y) + pos[:, :E], ONE fp32 add per element, so bit-exact; B in {1, 17}, N in {2, 5},
    pos NULL / ld_pos = E / ld_pos = E + 64 with NaN in the columns the kernel must not read into the result."""
    lib = _lib()
    for B in (1, 17):
        for N in (2, 5):
            g = _gen(E + 7 * B + N)
            y = torch.randn(B, N - 1, E, device=DEV, generator=g).bfloat16()
            cls = torch.randn(E, device=DEV, generator=g)
            for ld in (None, E, E + 64):
                pos = pos_full = None
                if ld is not None:
                    pos_full = torch.full((N, ld), NAN, device=DEV)
                    pos_full[:, :E] = torch.randn(N, E, device=DEV, generator=g)
                    pos = pos_full[:, :E]
                x0 = Guarded((B, N, E))
                rc = lib.cream_stem_assemble(_p(x0.t), _p(y), _p(cls), _p(pos_full), ld or 0, B, N, E, _stream())
                assert rc == OK
                torch.cuda.synchronize()
                assert x0.intact() and bool(torch.isfinite(x0.t).all())
                want = torch.cat([cls.expand(B, 1, E), y.float()], dim=1)
                if pos is not None:
                    want = want + pos
                assert torch.equal(x0.t, want), (B, N, E, ld)
                assert torch.equal(x0.t.double(), R.stem_assemble(y, cls, pos).float().double())


@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_stem_backward_chunk_sums_against_float64(B):
    """cream_stem_bwd: dy == bf16(dx0[:, 1:]) bit for bit; every one of the cream_stem_bwd_chunks(B) slabs of psum against the
    float64 sum over ITS images (one chunk, a full chunk, a one-image last chunk behind one and behind two full chunks), and
    psum.sum(0) against the sum over the batch; N in {2, 5}, E in {4, 36, 388} (N E / 4 below and no multiple of 256).
    Measured on the MI355X (ulp of the row's largest sum, worst over the cases): slabs kernel 1.69 / framework fp32 1.15,
    batch sum 1.67 / 1.10."""
    lib = _lib()
    chunks = lib.cream_stem_bwd_chunks(B)
    assert chunks == -(-B // 16)
    worst = {}
    for N in (2, 5):
        for E in (4, 36, 388):
            dx0 = torch.randn(B, N, E, device=DEV, generator=_gen(B * 100 + N * 10 + E)) * 0.5 + 2
            dy, psum = Guarded((B, N - 1, E), torch.bfloat16), Guarded((chunks, N, E))
            assert lib.cream_stem_bwd(_p(dy.t), _p(psum.t), _p(dx0), B, N, E, _stream()) == OK
            torch.cuda.synchronize()
            assert dy.intact() and psum.intact()
            assert bool(torch.isfinite(psum.t).all()) and bool(torch.isfinite(dy.t.float()).all())
            r_dy, r_psum = R.stem_bwd(dx0)
            assert torch.equal(_bits(dy.t), _bits(dx0[:, 1:].bfloat16())) and torch.equal(dy.t.double(), r_dy.float().bfloat16().double())
            fw = torch.stack([dx0[b0:b0 + 16].sum(0) for b0 in range(0, B, 16)])
            _hold(f"stem_bwd psum slabs @ B={B} N={N} E={E}", psum.t, fw, r_psum, worst=worst)
            _hold(f"stem_bwd psum batch sum @ B={B} N={N} E={E}", psum.t.double().sum(0), dx0.sum(0), dx0.double().sum(0), worst=worst)
    _report(f"B={B}", worst)


# ---- soft-target cross entropy ------------------------------------------------------------------------------------------
def _ce_run(lib, logits, target, gs):
    B, C = logits.shape
    code = 2 if logits.dtype == torch.bfloat16 else 0
    rows, dl = Guarded((B,)), Guarded((B, C))
    assert lib.cream_soft_ce(_p(rows.t), _p(dl.t), _p(logits), _p(target), B, C, code, gs, _stream()) == OK
    torch.cuda.synchronize()
    assert rows.intact() and dl.intact(), "sentinel band overwritten"
    assert bool(torch.isfinite(rows.t).all()) and bool(torch.isfinite(dl.t).all())
    return rows.t, dl.t


def _ce_framework(x32, target, gs):
    xr = x32.clone().requires_grad_()
    rows = torch.sum(-target * torch.log_softmax(xr, -1), -1)
    (gx,) = torch.autograd.grad(rows.sum() * gs, xr)
    return rows.detach(), gx


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 2, 255, 256, 257, 2048])
def test_soft_target_ce_against_float64_at_large_logits(C, dt):
    """cream_soft_ce with logits spread over +-80 (fp32) / +-60 (bf16) — exp overflows without the max subtraction —,
    target rows that sum to 1, 0.5 and 2 under grad_scale 1 / B (the `st` factor of the gradient), and one-hot targets with
    exact zeros under grad_scale 1, a -inf logit sitting at a zero-target class: loss and gradient stay finite and equal the
    reference with that class removed.  B = 3.
    Measured on the MI355X (worst over C and both dtypes): loss rows kernel 2.24 ulp / framework fp32 1.17 ulp of the value,
    dlogits 2.18 / 2.99 ulp of the row's largest gradient."""
    lib, B = _lib(), 3
    amp = 80.0 if dt == torch.float32 else 60.0
    g = _gen(C + (7 if dt == torch.float32 else 13))
    x = (torch.rand(B, C, device=DEV, generator=g) * 2 - 1) * amp
    x[:, 0] = amp
    if C >= 2:
        x[:, C // 2] = -amp
    logits = x.to(dt)
    x32 = logits.float()
    worst = {}
    # soft targets, rows summing to 1, 0.5 and 2
    target = torch.softmax(torch.randn(B, C, device=DEV, generator=g), -1) * torch.tensor([[1.0], [0.5], [2.0]], device=DEV)
    rows, dl = _ce_run(lib, logits, target, 1.0 / B)
    r_rows, r_dl = R.soft_ce(x32, target, 1.0 / B)
    fw_rows, fw_dl = _ce_framework(x32, target, 1.0 / B)
    _hold(f"soft_ce loss @ C={C} soft", rows, fw_rows, r_rows, floor="elem", worst=worst)
    _hold(f"soft_ce dlogits @ C={C} soft", dl, fw_dl, r_dl, worst=worst)
    # one-hot targets (exact zeros); from C = 2 on a -inf logit at a class whose target is zero
    hot_at = torch.tensor([0, C // 2, C - 1], device=DEV)
    cinf = 1 if C > 2 else C - 1
    if C == 2:
        hot_at = torch.zeros(B, dtype=torch.long, device=DEV)
    elif C > 2:
        hot_at = torch.where(hot_at == cinf, hot_at + 1, hot_at)
    hot = F.one_hot(hot_at, C).float()
    lg = logits.clone()
    keep = list(range(C))
    if C >= 2:
        lg[:, cinf] = float("-inf")
        keep.remove(cinf)
    rows, dl = _ce_run(lib, lg, hot, 1.0)
    xk, tk = lg.float()[:, keep], hot[:, keep]
    r_rows, r_dl = R.soft_ce(xk, tk, 1.0)
    fw_rows, fw_dl = _ce_framework(xk, tk, 1.0)
    _hold(f"soft_ce loss @ C={C} one-hot", rows, fw_rows, r_rows, floor="elem", worst=worst)
    _hold(f"soft_ce dlogits @ C={C} one-hot", dl[:, keep], fw_dl, r_dl, worst=worst)
    if C >= 2:
        assert float(dl[:, cinf].abs().max()) == 0.0
        full_rows, full_dl = R.soft_ce(lg.float(), hot, 1.0)              # the reference given the -inf itself
        assert torch.allclose(full_rows, r_rows, rtol=1e-13, atol=0) and float(full_dl[:, cinf].abs().max()) == 0.0
    _report(f"C={C} {dt}", worst)


def test_soft_ce_refuses_wide_rows_and_other_dtypes_without_launching():
    lib = _lib()
    rows, dl = Guarded((3,), fill=0.0), Guarded((3, 2049), fill=0.0)
    x, t = torch.zeros(3, 2049, device=DEV), torch.zeros(3, 2049, device=DEV)
    assert lib.cream_soft_ce(_p(rows.t), _p(dl.t), _p(x), _p(t), 3, 2049, 0, 1.0, _stream()) == TOO_LARGE
    for code in (1, 3, 7):                                               # f16, f64, no dtype at all
        assert lib.cream_soft_ce(_p(rows.t), _p(dl.t), _p(x), _p(t), 3, 256, code, 1.0, _stream()) == BAD_DTYPE
    torch.cuda.synchronize()
    assert float(dl.t.abs().max()) == 0.0 and float(rows.t.abs().max()) == 0.0 and dl.intact() and rows.intact()


# ---- AdamW + operand copies ---------------------------------------------------------------------------------------------
LR, BETA1, BETA2, EPS = 1e-2, 0.9, 0.999, 1e-8
# (name, rows, cols, ld, weight decay, has a gradient, de-interleave, ld_mir, ld_mir_t): ld_mir None = no row copy.
# Tile counts 1 1 1 1 4 9 1 2 4 4 4: single-tile jobs next to each other, then mixed ones (the search over first_tile).
ADAMW_JOBS = [
    ("1x1", 1, 1, 1, 0.0, True, False, None, None),                      # no copies
    ("1x37", 1, 37, 37, 0.05, True, False, 37, None),                    # row copy only, scalar stores (ld_mir = cols, odd)
    ("96x64", 96, 64, 64, 0.05, True, False, 72, 96),                    # one full tile; ld_mir = cols + 8, vector stores
    ("frozen40x20", 40, 20, 20, 0.05, False, False, 20, 40),             # g == NULL between two updated jobs
    ("97x65", 97, 65, 65, 0.0, True, False, 66, 101),                    # ld & 3, c + 4 > cols, ld_mir & 3, ld_mir_t & 7
    ("200x130", 200, 130, 130, 0.05, True, False, 130, 200),             # ld & 3 == 2; transposed copy: vector + row tail
    ("33x4", 33, 4, 4, 0.0, True, False, 12, 37),                        # ld_mir = cols + 8, ld_mir_t = rows + 4
    ("50x72ld96", 50, 72, 96, 0.05, True, False, 80, 56),                # a (50, 72) view of a (50, 96) tensor
    ("qkv120x72", 120, 72, 72, 0.05, True, True, 72, 40),                # row tail inside a de-interleaved tile
    ("qkv303x64", 303, 64, 64, 0.0, True, True, 72, 104),                # padded copies of the three parts
    ("qkv120x72s", 120, 72, 72, 0.0, True, True, 74, 44),                # the same through the scalar stores
]


class _AdamwProblem:
    def __init__(self, seed, moments):
        from cream_amd.autoformer import block as K
        self.lib = _lib()
        g = _gen(seed)
        self.gen = g
        self.jobs, cjobs = [], []
        for name, rows, cols, ld, wd, has_g, deint, ld_mir, ld_mir_t in ADAMW_JOBS:
            j = dict(name=name, rows=rows, cols=cols, ld=ld, wd=wd, has_g=has_g, deint=deint, ld_mir=ld_mir, ld_mir_t=ld_mir_t)
            sign = lambda: torch.where(torch.rand(rows, cols, device=DEV, generator=g) < 0.5, -1.0, 1.0)   # noqa: E731
            j["p"], j["g"], j["m"], j["v"] = (Guarded((rows, ld)) for _ in range(4))
            j["p"].t[:, :cols] = sign() * (0.5 + torch.rand(rows, cols, device=DEV, generator=g))   # |p| in [0.5, 1.5): no cancellation
            j["gsign"] = sign()
            j["m"].t.fill_(SENT)
            j["v"].t.fill_(SENT)
            if moments:
                j["m"].t[:, :cols] = j["gsign"] * 0.05 * (0.5 + torch.rand(rows, cols, device=DEV, generator=g))
                j["v"].t[:, :cols] = (0.1 * (0.5 + torch.rand(rows, cols, device=DEV, generator=g))) ** 2
            else:
                j["m"].t[:, :cols] = 0.0
                j["v"].t[:, :cols] = 0.0
            flat = lambda b: b.t.view(-1)[:rows * cols].view(rows, cols)  # noqa: E731  same pointer, the shape param_job wants
            mir = mir_t = None
            q = rows // 3 if deint else rows
            if ld_mir is not None:
                j["mir"] = Guarded((3, q, ld_mir) if deint else (rows, ld_mir), torch.bfloat16, fill=SENT)
                mir = j["mir"].t[..., :cols]
            if ld_mir_t is not None:
                j["mir_t"] = Guarded((3, cols, ld_mir_t) if deint else (cols, ld_mir_t), torch.bfloat16, fill=SENT)
                mir_t = j["mir_t"].t[..., :q]
            j["mir_v"], j["mir_t_v"] = mir, mir_t
            cj = K.param_job(flat(j["p"]), flat(j["g"]) if has_g else None, flat(j["m"]), flat(j["v"]), mir, mir_t,
                             deinterleave=deint, weight_decay=wd)
            cj.ld = ld                                                   # param_job assumes a contiguous tensor
            assert (cj.rows, cj.cols) == (rows, cols)
            if mir is not None:
                assert cj.ld_mir == ld_mir and cj.seg_stride == (q * ld_mir if deint else 0)
            if mir_t is not None:
                assert cj.ld_mir_t == ld_mir_t and cj.seg_stride_t == (cols * ld_mir_t if deint else 0)
            self.jobs.append(j)
            cjobs.append(cj)
        self.table = K.JobTable(cjobs, torch.device(DEV))
        # the framework's fp32 AdamW and the float64 reference start from the same values
        for j in self.jobs:
            c = j["cols"]
            j["q"] = torch.nn.Parameter(j["p"].t[:, :c].clone())
            j["ref"] = [j["p"].t[:, :c].double(), j["m"].t[:, :c].double(), j["v"].t[:, :c].double()]
        groups = [dict(params=[j["q"] for j in self.jobs if j["has_g"] and j["wd"] == wd], weight_decay=wd) for wd in (0.0, 0.05)]
        self.opt = torch.optim.AdamW(groups, lr=LR, betas=(BETA1, BETA2), eps=EPS, foreach=False)
        if moments:
            for j in self.jobs:
                if j["has_g"]:
                    self.opt.state[j["q"]] = dict(step=torch.tensor(float(moments)), exp_avg=j["ref"][1].float().clone(),
                                                  exp_avg_sq=j["ref"][2].float().clone())
        self.pad_before = [{k: _bits(j[k].whole).clone() for k in ("p", "m", "v")} for j in self.jobs]

    def new_gradients(self):
        """Fixed signs; every 7th element exactly zero (v stays 0 from zero moments: eps decides), others 1e-12 and 1e3."""
        for j in self.jobs:
            rows, cols = j["rows"], j["cols"]
            gr = j["gsign"] * 0.1 * (0.5 + torch.rand(rows, cols, device=DEV, generator=self.gen))
            idx = torch.arange(rows * cols, device=DEV).view(rows, cols)
            gr = torch.where(idx % 11 == 1, j["gsign"] * 1e-12, gr)
            gr = torch.where(idx % 13 == 2, j["gsign"] * 1e3, gr)
            gr = torch.where(idx % 7 == 0, torch.zeros_like(gr), gr)
            j["g"].t[:, :cols] = gr
            j["q"].grad = gr.clone() if j["has_g"] else None
            j["gr"] = gr

    def step(self, step, worst):
        self.new_gradients()
        before = [_bits(j["p"].whole).clone() for j in self.jobs]
        self.table.launch(update=True, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS, step=step)
        torch.cuda.synchronize()
        self.opt.step()
        for j, b in zip(self.jobs, before):
            c, name = j["cols"], j["name"]
            if not j["has_g"]:
                assert torch.equal(_bits(j["p"].whole), b), f"{name}: a job without gradient was updated"
                continue
            j["ref"] = list(R.adamw_step(*([j["ref"][0], j["gr"]] + j["ref"][1:]), LR, BETA1, BETA2, EPS, j["wd"], step))
            st = self.opt.state[j["q"]]
            for what, buf, fw, ref in (("p", j["p"], j["q"].detach(), j["ref"][0]), ("m", j["m"], st["exp_avg"], j["ref"][1]),
                                       ("v", j["v"], st["exp_avg_sq"], j["ref"][2])):
                _hold(f"adamw {what} @ {name} step {step}", buf.t[:, :c], fw, ref, floor="elem", worst=worst)
            zero = j["gr"] == 0
            if step <= 3:                                                # from zero moments: the eps branch, exactly
                assert float(j["v"].t[:, :c][zero].abs().max() if zero.any() else 0.0) == 0.0
        self.check_untouched(("m", "v", "p"), padding_only=True)
        self.check_copies()

    def check_untouched(self, which, padding_only):
        """Sentinel bands and the columns cols..ld of p / m / v (or, padding_only False, every bit of them)."""
        for j, b in zip(self.jobs, self.pad_before):
            for k in which:
                assert j[k].intact(), f"{j['name']}: band behind {k} overwritten"
                now = _bits(j[k].whole)
                if padding_only:
                    if j["ld"] > j["cols"]:
                        pad = lambda t: t[:j["rows"] * j["ld"]].view(j["rows"], j["ld"])[:, j["cols"]:]   # noqa: E731
                        assert torch.equal(pad(now), pad(b[k])), f"{j['name']}: columns cols..ld of {k} touched"
                else:
                    assert torch.equal(now, b[k]), f"{j['name']}: {k} changed"
            assert j["g"].intact()

    def check_copies(self):
        """mir / mir_t == bf16 of the kernel's own p (de-interleaved: super row 3 i + j -> part j, row i), padding untouched."""
        for j in self.jobs:
            name, c = j["name"], j["cols"]
            want = j["p"].t[:, :c].bfloat16()
            if j["deint"]:
                want = R.deinterleave(want)
            q = want.shape[-2]
            if j["mir_v"] is not None:
                assert j["mir"].intact(), f"{name}: band behind mir overwritten"
                assert torch.equal(_bits(j["mir_v"]), _bits(want)), f"{name}: mir != bf16(p)"
                assert bool((j["mir"].t[..., c:] == SENT).all()), f"{name}: columns cols..ld_mir of mir touched"
            if j["mir_t_v"] is not None:
                assert j["mir_t"].intact(), f"{name}: band behind mir_t overwritten"
                assert torch.equal(_bits(j["mir_t_v"]), _bits(want.transpose(-1, -2))), f"{name}: mir_t != bf16(p)^T"
                assert bool((j["mir_t"].t[..., q:] == SENT).all()), f"{name}: rows nrows..ld_mir_t of mir_t touched"

    def poison_copies(self):
        for j in self.jobs:
            if j["mir_v"] is not None:
                j["mir_v"].fill_(NAN)
            if j["mir_t_v"] is not None:
                j["mir_t_v"].fill_(NAN)


def test_adamw_job_tiles_and_prefix_sums():
    lib = _lib()
    pb = _AdamwProblem(1, None)
    tiles = [lib.cream_param_job_tiles(j["rows"], j["cols"]) for j in pb.jobs]
    assert tiles == [-(-j["rows"] // 96) * -(-j["cols"] // 64) for j in pb.jobs] == [1, 1, 1, 1, 4, 9, 1, 2, 4, 4, 4]
    first = [0]
    for t in tiles:
        first.append(first[-1] + t)
    assert pb.table.first.cpu().tolist() == first and pb.table.total == first[-1] and pb.table.n == len(pb.jobs) >= 8
    assert lib.cream_param_job_tiles(0, 5) == 0 and lib.cream_param_job_tiles(97, 65) == 4


def test_adamw_steps_one_to_three_from_zero_moments_against_float64():
    """cream_adamw_step over 11 synthetic jobs in ONE launch (scalar and vector paths of the update and of both copies, a
    strided tensor, de-interleaved tensors whose row tail falls inside a tile, a g == NULL job between updated ones, weight
    decay 0 and 0.05; gradients exactly zero, 1e-12 and 1e3 among ordinary ones): p, m, v after steps 1, 2, 3 elementwise
    against the float64 AdamW, the fp32 baseline being torch.optim.AdamW(foreach=False); the copies equal bf16 of the kernel's
    own p bit for bit; padding and sentinel bands untouched.
    Measured on the MI355X (ulp of each value, worst over jobs and steps; kernel / torch fp32): p 2.78 / 2.78,
    m 1.17 / 0.98, v 2.02 / 1.99."""
    pb = _AdamwProblem(2, None)
    worst = {}
    for step in (1, 2, 3):
        pb.poison_copies()
        pb.step(step, worst)
    _report("steps 1..3", worst)


def test_adamw_late_step_from_given_moments_against_float64():
    """One launch with step = 1000 (bias corrections 1 - 0.9^1000 = 1 and 1 - 0.999^1000 = 0.632) from non-zero m, v.
    Measured on the MI355X (kernel / torch fp32, ulp of each value): p 1.15 / 1.15, m 0.92 / 0.69, v 1.08 / 1.08."""
    pb = _AdamwProblem(3, 999)
    worst = {}
    pb.poison_copies()
    pb.step(1000, worst)
    _report("step 1000", worst)


def test_adamw_copy_mode_leaves_the_master_tensors_alone():
    """update = 0: p, m, v bit-identical before and after (padding and bands included), every copy written."""
    pb = _AdamwProblem(4, 999)
    pb.new_gradients()
    pb.pad_before = [{k: _bits(j[k].whole).clone() for k in ("p", "m", "v")} for j in pb.jobs]
    pb.poison_copies()
    pb.table.launch(update=False)
    torch.cuda.synchronize()
    pb.check_untouched(("p", "m", "v"), padding_only=False)
    pb.check_copies()
