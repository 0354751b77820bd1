"""Plain float64 restatements of the header contracts (include/cream_amd.h) of the kernels at the two ends of the
training step: csrc/stem_tail.hip (im2patch, stem assemble / backward, tail forward / backward, soft-target cross
entropy) and csrc/optim.hip (AdamW + the bf16 operand copies).  Every function takes tensors of any dtype and device,
computes in float64 on that device and shares no code with the kernels.  tests/test_ends_ref_cpu.py pins them against
the framework's own float64 operators; tests/test_ends_gpu.py holds the kernels to them."""
import math

import torch

ULP32 = 2.0 ** -23          # spacing of fp32 numbers relative to a value in [1, 2)


# ---- stem ---------------------------------------------------------------------------------------------------------
def unfold(img, ph, pw):
    """patches (B * gh * gw, C * ph * pw): patch (b, gi, gj) in row-major order, elements in (c, i, j) order."""
    B, C, H, W = img.shape
    gh, gw = H // ph, W // pw
    x = img.reshape(B, C, gh, ph, gw, pw).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B * gh * gw, C * ph * pw)


def stem_assemble(y, cls, pos):
    """x0 (B, N, E): row 0 = cls + pos[0], row n = y[:, n - 1] + pos[n]; y (B, N - 1, E), cls (E), pos (N, E) or None."""
    B, _, E = y.shape
    x0 = torch.cat([cls.double().reshape(1, 1, E).expand(B, 1, E), y.double()], dim=1)
    return x0 if pos is None else x0 + pos.double()[None]


def stem_bwd(dx0, per_chunk=16):
    """dy = dx0[:, 1:] (the caller rounds it) and psum (chunks, N, E): sums of dx0 over chunks of `per_chunk` images."""
    B = dx0.shape[0]
    d = dx0.double()
    psum = torch.stack([d[b0:b0 + per_chunk].sum(0) for b0 in range(0, B, per_chunk)])
    return d[:, 1:], psum


# ---- tail ---------------------------------------------------------------------------------------------------------
def pending(x1, f, sample_scale):
    """The stream the last block hands over: x1 + s_b * f (f may be None; the scale counts only with f)."""
    x = x1.double()
    if f is not None:
        s = sample_scale.double()[:, None, None] if sample_scale is not None else 1.0
        x = x + s * f.double()
    return x


def layer_norm_rows(x, eps):
    """xhat, mean, rstd over the last dimension with the biased variance (two passes in float64)."""
    mean = x.mean(-1)
    d = x - mean[..., None]
    rstd = (d.pow(2).mean(-1) + eps).rsqrt()
    return d * rstd[..., None], mean, rstd


def tail_fwd(x1, f, sample_scale, gamma, beta, eps):
    """pooled (B, E) = mean over tokens n >= 1 of LayerNorm(x1 + s_b f) * gamma + beta; xm = that mean before the affine
    map; mean, rstd (B, N) of every row, the class token's included."""
    xhat, mean, rstd = layer_norm_rows(pending(x1, f, sample_scale), eps)
    xm = xhat[:, 1:].mean(1)
    return xm * gamma.double() + beta.double(), xm, mean, rstd


def tail_bwd(g, x1, f, sample_scale, gamma, beta, eps):
    """dx (B, N, E) = d sum(pooled * g) / d (x1 + s_b f) by float64 autograd, and s_b * dx (the gradient of f before its
    rounding to bf16; sample_scale None = 1)."""
    x = pending(x1, f, sample_scale).detach().requires_grad_()
    xhat, _, _ = layer_norm_rows(x, eps)
    pooled = xhat[:, 1:].mean(1) * gamma.double() + beta.double()
    (dx,) = torch.autograd.grad(pooled, x, g.double())
    s = sample_scale.double()[:, None, None] if sample_scale is not None else 1.0
    return dx, dx * s


# ---- soft-target cross entropy --------------------------------------------------------------------------------------
def soft_ce(logits, target, grad_scale):
    """loss_rows (B) = sum_c -t log_softmax(x)[c] and dlogits = (softmax(x) sum_c t - t) * grad_scale.  Written out with
    an explicit maximum so that neither exp overflows; classes with x = -inf and t = 0 contribute nothing."""
    x, t = logits.double(), target.double()
    mx = x.max(-1, keepdim=True).values
    e = torch.exp(x - mx)
    se = e.sum(-1, keepdim=True)
    lse = mx + se.log()
    terms = torch.where(t == 0, torch.zeros_like(t), t * (lse - x))
    loss = terms.sum(-1)
    dl = (e / se * t.sum(-1, keepdim=True) - t) * grad_scale
    return loss, dl


# ---- AdamW ----------------------------------------------------------------------------------------------------------
def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    """One step of AdamW (decoupled weight decay, bias-corrected moments, no amsgrad).  Returns new (p, m, v)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    p = p * (1.0 - lr * weight_decay)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def deinterleave(w):
    """(3 Q, cols) -> (3, Q, cols): super row 3 i + j goes to part j, row i."""
    rows, cols = w.shape
    return w.reshape(rows // 3, 3, cols).permute(1, 0, 2)


# ---- the tolerance rule -----------------------------------------------------------------------------------------------
def row_floor(ref, ulps=4.0):
    """`ulps` fp32 ulps of the largest reference magnitude of each row (last dimension), broadcast over the row."""
    r = ref.double().abs()
    top = r.amax(-1, keepdim=True) if r.dim() else r
    return (ulps * ULP32 * top).expand_as(r)


def elem_floor(ref, ulps=4.0):
    """`ulps` fp32 ulps of every reference value itself."""
    return ulps * ULP32 * ref.double().abs()


def ulps_of_floor(a, ref, floor, ulps=4.0):
    """Largest |a - ref| in units of one ulp of the floor's scale (elements whose floor is 0 must match exactly)."""
    err = (a.double() - ref.double()).abs()
    q = torch.where(floor > 0, err / (floor / ulps).clamp_min(1e-300),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(q.max()) if q.numel() else 0.0


def check_against_fp32_baseline(kernel, baseline, ref, floor="row", margin=4.0):
    """The rule of the suite for fp32 sums and transcendental functions.  `baseline` is the framework's fp32 evaluation
    of the same formula on the same inputs, `ref` the float64 one.  At EVERY element
        |kernel - ref| <= margin * (the framework's error) + floor,      floor = 4 fp32 ulp,
    in one of two scales:
      floor = "elem"  for element-wise formulas (the optimizer, rstd, a loss value): everything relative to the element,
                      |kernel - ref| <= (margin * tol_fw + 4 ulp) * |ref|,  tol_fw = max_i |baseline - ref| / |ref|
                      (where ref is 0 and the baseline is exact, the kernel must be exact);
      floor = "row"   for sums (also a tensor of absolute floors, one per row): the error of an fp32 sum lives on the
                      scale of its terms, not of a result that cancellation made small, so both the floor (4 ulp of the
                      row's largest reference magnitude) and the framework's error (its largest |baseline - ref| in
                      that row, last dimension) are per row — a relative tolerance fitted at one small element would
                      say nothing about the others.
    The margin covers another legitimate summation order; a dropped term costs about 1 / E of the row's scale.
    Returns (ok, kernel error, framework error), both as the largest |. - ref| in ulp of the floor's scale."""
    ref = ref.double()
    err_fw = (baseline.double() - ref).abs()
    if isinstance(floor, str) and floor == "elem":
        fl = elem_floor(ref)
        rel = torch.where(err_fw > 0, err_fw / ref.abs().clamp_min(1e-300), torch.zeros_like(err_fw))
        allowance = (float(rel.max()) if rel.numel() else 0.0) * ref.abs()
    else:
        fl = floor.double().expand_as(ref) if torch.is_tensor(floor) else row_floor(ref)
        allowance = (err_fw.amax(-1, keepdim=True) if ref.dim() else err_fw).expand_as(ref)
    u_fw = ulps_of_floor(baseline, ref, fl)
    if kernel.shape != ref.shape or not bool(torch.isfinite(kernel.double()).all()):
        return False, float("inf"), u_fw
    ok = bool(((kernel.double() - ref).abs() <= margin * allowance + fl).all())
    return ok, ulps_of_floor(kernel, ref, fl), u_fw
