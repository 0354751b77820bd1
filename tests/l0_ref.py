"""References, rounding bounds and injected faults for TinyCLIP's mask folding (cream_amd/csrc/l0_mask.hip,
cream_amd/tinyclip/native_masked.py), shared by tests/test_l0_ref_cpu.py and tests/test_l0_kernel_gpu.py.

  * `folded_tower` — the algebra in fp64: a masked block IS the dense block on the effective operands
        Wo' = diag(zh) Wo diag(e(zd)),  bo' = zh * bo,  W2' = diag(zh) W2 diag(zi),  b2' = zh * b2
    with the masked LayerNorm for ln_1 / ln_2; the weight and mask gradients follow from the gradients of the effective
    operands at weight size (`unfold_gradients`).  Written from the formulas, with nothing of cream_amd/tinyclip/model.py.
  * `ln_fwd_ref` / `ln_bwd_ref`, `pack_ref`, `finalize_ref` — what the three kernel groups compute, in fp64 (the pack: the
    same fp32 products rounded by torch, bit for bit), each with a per-element bound derived from the number of fp32
    operations (unit roundoff U32 = 2^-24 each, gamma_k = k U32 / (1 - k U32) for k of them in any order) and the single bf16
    rounding (U16 = 2^-8, relative to the value rounded) — no fitted constant.
  * `*_model` — the kernels' arithmetic in fp32 on the CPU with a fault on request (FAULTS): the CPU test shows that the
    model passes every bound and that every fault breaks one.
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U16 = 2.0 ** -8          # bf16: 8 significant bits, round to nearest
HEAD = 64

FAULTS = ("dropped_in_stats", "divisor_E", "rc_swapped", "last_part_skipped", "c_group_ignored")


def gamma(k):
    return k * U32 / (1.0 - k * U32)


# ---- the algebra (fp64) ----------------------------------------------------------------------------------------------
def masked_ln(x, w, b, z, eps=1e-5):
    """Statistics over the columns with z != 0, divisor n_keep; exact zeros elsewhere; no dependence on the values of z."""
    keep = z != 0
    out = torch.zeros_like(x)
    out[..., keep] = F.layer_norm(x[..., keep], [int(keep.sum())], w[keep], b[keep], eps)
    return out


def dense_block(x, p, zh, heads, causal):
    """One pre-LayerNorm block (TinyCLIP model.py:285-315 without any mask on the branches) on the operands in `p`, with the
    masked LayerNorm.  x (N, L, D)."""
    N, L, D = x.shape
    a = masked_ln(x, p["ln_1.weight"], p["ln_1.bias"], zh)
    qkv = a @ p["wqkv"].T + p["bqkv"]
    q, k, v = qkv.view(N, L, 3, heads, HEAD).permute(2, 0, 3, 1, 4).unbind(0)
    s = (q * HEAD ** -0.5) @ k.transpose(-2, -1)
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=x.dtype).triu_(1)
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(N, L, heads * HEAD)
    x = x + o @ p["wo"].T + p["bo"]
    c = masked_ln(x, p["ln_2.weight"], p["ln_2.bias"], zh)
    return x + F.gelu(c @ p["w1"].T + p["b1"]) @ p["w2"].T + p["b2"]


def block_params(blk):
    """The tensors of one ResidualAttentionBlock as fp64 leaves (any module with the reference's parameter names)."""
    sd = {k: v.detach().double().clone().requires_grad_() for k, v in blk.named_parameters()}
    return {"ln_1.weight": sd["ln_1.weight"], "ln_1.bias": sd["ln_1.bias"], "ln_2.weight": sd["ln_2.weight"], "ln_2.bias": sd["ln_2.bias"],
            "wqkv": sd["attn.in_proj_weight"], "bqkv": sd["attn.in_proj_bias"], "wo": sd["attn.out_proj.weight"],
            "bo": sd["attn.out_proj.bias"], "w1": sd["mlp.c_fc.weight"], "b1": sd["mlp.c_fc.bias"], "w2": sd["mlp.c_proj.weight"],
            "b2": sd["mlp.c_proj.bias"]}


NAMES = {"wqkv": "attn.in_proj_weight", "bqkv": "attn.in_proj_bias", "wo": "attn.out_proj.weight", "bo": "attn.out_proj.bias",
         "w1": "mlp.c_fc.weight", "b1": "mlp.c_fc.bias", "w2": "mlp.c_proj.weight", "b2": "mlp.c_proj.bias"}


def effective(p, zh, zd, zi):
    """The effective operands of a block as NEW leaves (their gradients are dW' of the issue's algebra)."""
    e = zd.repeat_interleave(HEAD)
    q = dict(p)
    q["wo"] = (zh[:, None] * p["wo"] * e[None, :]).detach().requires_grad_()
    q["bo"] = (zh * p["bo"]).detach().requires_grad_()
    q["w2"] = (zh[:, None] * p["w2"] * zi[None, :]).detach().requires_grad_()
    q["b2"] = (zh * p["b2"]).detach().requires_grad_()
    return q


def unfold_gradients(p, q, zh, zd, zi):
    """From the gradients of the effective operands (q[..].grad) at weight size: the gradients of Wo, bo, W2, b2 and this
    block's contributions to d zd, d zi, d zh."""
    e = zd.repeat_interleave(HEAD)
    gwo, gbo, gw2, gb2 = q["wo"].grad, q["bo"].grad, q["w2"].grad, q["b2"].grad
    out = {"wo": zh[:, None] * e[None, :] * gwo, "bo": zh * gbo, "w2": zh[:, None] * zi[None, :] * gw2, "b2": zh * gb2}
    dzd = (gwo * p["wo"] * zh[:, None]).sum(0).view(-1, HEAD).sum(1)
    dzi = (gw2 * p["w2"] * zh[:, None]).sum(0)
    dzh = (gwo * p["wo"] * e[None, :]).sum(1) + gbo * p["bo"] + (gw2 * p["w2"] * zi[None, :]).sum(1) + gb2 * p["b2"]
    return out, dzd, dzi, dzh


def folded_tower(blocks, x, gy, zh, zd, zi, heads, causal):
    """The run of blocks through the folding.  -> (y, dx, {parameter name: gradient} per block, dzh (D), dzd (layers, H),
    dzi (layers, F)); everything fp64."""
    x = x.detach().double().requires_grad_()
    ps = [block_params(b) for b in blocks]
    qs = [effective(p, zh, zd[i], zi[i]) for i, p in enumerate(ps)]
    y = x
    for q in qs:
        y = dense_block(y, q, zh, heads, causal)
    y.backward(gy.double())
    grads, dzh, dzds, dzis = [], torch.zeros_like(zh), [], []
    for i, (p, q) in enumerate(zip(ps, qs)):
        un, dzd, dzi, dh = unfold_gradients(p, q, zh, zd[i], zi[i])
        g = {NAMES.get(k, k): (un[k] if k in un else q[k].grad) for k in p}
        grads.append(g)
        dzh = dzh + dh
        dzds.append(dzd)
        dzis.append(dzi)
    return y.detach(), x.grad, grads, dzh, torch.stack(dzds), torch.stack(dzis)


# ---- a. masked LayerNorm ------------------------------------------------------------------------------------------------
KEEP_PATTERNS = ("all", "first_dropped", "last_dropped", "group8_dropped", "every_second", "single_kept")


def keep_pattern(name, E):
    z = torch.rand(E, generator=torch.Generator().manual_seed(E)) * 0.9 + 0.1       # kept entries: any non-zero value
    if name == "first_dropped":
        z[0] = 0
    elif name == "last_dropped":
        z[-1] = 0
    elif name == "group8_dropped":
        z[8 * (E // 16):8 * (E // 16) + 8] = 0
    elif name == "every_second":
        z[1::2] = 0
    elif name == "single_kept":
        z[:] = 0
        z[(3 * E) // 4 + 1] = 0.5
    return z


def ln_case(M, E, pattern, with_res, seed=0, rows_per_sample=None):
    """fp32 / bf16 inputs of the forward; the dropped columns of x hold +-1e30."""
    g = torch.Generator().manual_seed(seed + 7 * M + E)
    z = keep_pattern(pattern, E)
    x = torch.randn(M, E, generator=g) * 2 + 0.5
    big = torch.where(torch.rand(M, E, generator=g) < 0.5, -1e30, 1e30)
    x = torch.where(z != 0, x, big.float())
    c = dict(x=x, z=z, gamma=1 + 0.2 * torch.randn(E, generator=g), beta=0.1 * torch.randn(E, generator=g), eps=1e-5, res=None, scale=None,
             rows_per_sample=rows_per_sample or max(1, M // 3))
    if with_res:
        c["res"] = torch.randn(M, E, generator=g).bfloat16()
        c["scale"] = torch.rand((M + c["rows_per_sample"] - 1) // c["rows_per_sample"], generator=g) * 2
    return c


def _row_scale(c, M):
    if c["res"] is None:
        return None
    return c["scale"][torch.arange(M) // c["rows_per_sample"]][:, None]


def ln_fwd_ref(c):
    """-> dict(xsum, y, mean, rstd) fp64 and the bounds dict(y, mean, rstd, xsum) (per element / per row)."""
    x, z = c["x"].double(), c["z"]
    M, E = x.shape
    keep = z != 0
    n = int(keep.sum())
    mag = x.abs()
    if c["res"] is not None:
        t = _row_scale(c, M).double() * c["res"].double()
        x, mag = x + t, mag + t.abs()
    xk, magk = x[:, keep], mag[:, keep]
    mean = xk.mean(1)
    d = xk - mean[:, None]
    var = (d * d).mean(1)
    rstd = (var + c["eps"]).rsqrt()
    gk, bk = c["gamma"].double()[keep], c["beta"].double()[keep]
    y = torch.zeros_like(x)
    y[:, keep] = d * rstd[:, None] * gk + bk
    # bounds.  xsum: one product, one sum.  mean: the inputs' error, n - 1 additions in any order, the reciprocal of n and the
    # product with it.  d: the input's error, the mean's, one subtraction.  var: d's error through d^2, a square, n - 1
    # additions, two products.  rstd: var's error through the monotone rsqrt, the addition of eps, rsqrtf itself (2 ulp).
    e_in = gamma(2) * magk if c["res"] is not None else torch.zeros_like(magk)
    e_mean = e_in.mean(1) + gamma(n + 2) * magk.mean(1)
    e_d = e_in + e_mean[:, None] + U32 * (d.abs() + e_in + e_mean[:, None])
    e_var = ((2 * d.abs() + e_d) * e_d).mean(1) + gamma(n + 3) * ((d.abs() + e_d) ** 2).mean(1)
    lo = (var - e_var).clamp_min(0) + c["eps"]
    e_rstd = (lo.rsqrt() - rstd).abs() + 8 * U32 * lo.rsqrt()
    pre = gk.abs() * (d.abs() * e_rstd[:, None] + (rstd + e_rstd)[:, None] * e_d) + gamma(3) * (y[:, keep].abs() + bk.abs())
    e_y = torch.zeros_like(x)
    e_y[:, keep] = pre + U16 * (y[:, keep].abs() + pre)
    return dict(xsum=x, y=y, mean=mean, rstd=rstd), dict(y=e_y, mean=e_mean, rstd=e_rstd, xsum=gamma(2) * mag)


def ln_fwd_model(c, fault=None):
    """The forward's arithmetic in fp32 (torch's summation order) -> dict(xsum, y (bf16), mean, rstd)."""
    x, z = c["x"], c["z"]
    M, E = x.shape
    keep = z != 0
    if c["res"] is not None:
        x = x + _row_scale(c, M) * c["res"].float()
    sel = torch.ones(E, dtype=torch.bool) if fault == "dropped_in_stats" else keep
    div = float(E) if fault == "divisor_E" else float(sel.sum())
    mean = x[:, sel].sum(1) / div
    d = x - mean[:, None]
    var = (d[:, sel] ** 2).sum(1) / div
    rstd = (var + c["eps"]).rsqrt()
    y = torch.where(keep, d * rstd[:, None] * c["gamma"] + c["beta"], torch.zeros(()))
    return dict(xsum=x, y=y.bfloat16(), mean=mean, rstd=rstd)


def check_ln_fwd(out, c):
    """Asserts the forward's outputs against the reference within the bounds; exact zeros in the dropped columns."""
    ref, bnd = ln_fwd_ref(c)
    keep = c["z"] != 0
    y = out["y"].double().cpu()
    assert bool((y[:, ~keep] == 0).all()), "a dropped column of y is not exactly 0"
    worst = {}
    for k in ("y", "mean", "rstd") + (("xsum",) if c["res"] is not None else ()):
        got, want, b = out[k].double().cpu(), ref[k], bnd[k]
        if k == "y":                                                    # (its dropped columns were held to exact zero above)
            got, want, b = got[:, keep], want[:, keep], b[:, keep]
        ratio = ((got - want).abs() / b.clamp_min(1e-300)).max()
        worst[k] = float(ratio)
        assert bool(((got - want).abs() <= b).all()), f"{k}: {float(ratio):.2f} x its bound"
    if c["res"] is not None:                                            # the stream itself passes in EVERY column
        assert bool(torch.isfinite(out["xsum"].cpu()).all())
    return worst


def ln_bwd_case(c, with_dres, with_scaled, seed=0):
    """The backward's inputs on top of a forward case: the statistics are the fp64 reference's rounded to fp32 — inputs."""
    g = torch.Generator().manual_seed(seed + 13)
    ref, _ = ln_fwd_ref(c)
    M, E = c["x"].shape
    b = dict(c)
    b["xin"] = ref["xsum"].float()                                      # (dropped columns: +-1e30 as they are)
    b["mean"], b["rstd"] = ref["mean"].float(), ref["rstd"].float()
    b["dy"] = torch.randn(M, E, generator=g).bfloat16()                 # non-zero in the dropped columns too: must be discarded
    b["dres"] = torch.randn(M, E, generator=g) if with_dres else None
    b["bscale"] = torch.rand((M + c["rows_per_sample"] - 1) // c["rows_per_sample"], generator=g) * 2 if with_scaled else None
    b["want_scaled"] = with_scaled
    return b


def ln_bwd_ref(b):
    """-> dict(dx, dxs, dgamma, dbeta) fp64 from the GIVEN fp32 statistics, and their bounds."""
    x, z = b["xin"].double(), b["z"]
    M, E = x.shape
    keep = z != 0
    n = int(keep.sum())
    mu, rs = b["mean"].double()[:, None], b["rstd"].double()[:, None]
    gk = b["gamma"].double()[keep]
    dy = b["dy"].double()[:, keep]
    xh = (x[:, keep] - mu) * rs
    dg = dy * gk
    s1, s2 = dg.mean(1, keepdim=True), (dg * xh).mean(1, keepdim=True)
    term = rs * (dg - s1 - xh * s2)
    dres = b["dres"].double() if b["dres"] is not None else torch.zeros_like(x)
    dx = dres.clone()
    dx[:, keep] += term
    sc = b["bscale"].double()[torch.arange(M) // b["rows_per_sample"]][:, None] if b["bscale"] is not None else torch.ones(M, 1, dtype=torch.float64)
    # bounds: xh two operations; dg one; s1 / s2 a sum of n terms of (1 / 3)-operation values, the reciprocal, a product
    e_xh = gamma(2) * xh.abs()
    e_s1 = gamma(n + 3) * dg.abs().mean(1, keepdim=True)
    e_s2 = gamma(n + 6) * (dg * xh).abs().mean(1, keepdim=True) + (dg.abs() * e_xh).mean(1, keepdim=True)
    e_term = rs * (U32 * dg.abs() + e_s1 + xh.abs() * e_s2 + s2.abs() * e_xh + gamma(4) * (dg.abs() + s1.abs() + (xh * s2).abs()))
    e_dx = torch.zeros_like(x)
    e_dx[:, keep] = e_term + U32 * (dres[:, keep].abs() + term.abs() + e_term)
    e_dxs = sc * e_dx + U32 * (sc * dx).abs()
    e_dxs = e_dxs + U16 * ((sc * dx).abs() + e_dxs)
    dgamma, dbeta = torch.zeros(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    dgamma[keep], dbeta[keep] = (dy * xh).sum(0), dy.sum(0)
    e_dgamma, e_dbeta = torch.zeros(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    e_dgamma[keep] = gamma(M + 8) * (dy * xh).abs().sum(0) + (dy.abs() * e_xh).sum(0)
    e_dbeta[keep] = gamma(M + 8) * dy.abs().sum(0)
    return dict(dx=dx, dxs=sc * dx, dgamma=dgamma, dbeta=dbeta), dict(dx=e_dx, dxs=e_dxs, dgamma=e_dgamma, dbeta=e_dbeta)


def ln_bwd_model(b, fault=None):
    x, z = b["xin"], b["z"]
    M, E = x.shape
    keep = z != 0
    sel = torch.ones(E, dtype=torch.bool) if fault == "dropped_in_stats" else keep
    div = float(E) if fault == "divisor_E" else float(sel.sum())
    mu, rs = b["mean"][:, None], b["rstd"][:, None]
    xh = torch.where(sel, (x - mu) * rs, torch.zeros(()))
    dg = torch.where(sel, b["dy"].float() * b["gamma"], torch.zeros(()))
    s1, s2 = dg.sum(1, keepdim=True) / div, (dg * xh).sum(1, keepdim=True) / div
    term = torch.where(keep, rs * (dg - s1 - xh * s2), torch.zeros(()))
    dx = (b["dres"] if b["dres"] is not None else 0) + term
    sc = b["bscale"][torch.arange(M) // b["rows_per_sample"]][:, None] if b["bscale"] is not None else 1.0
    dyk = torch.where(keep, b["dy"].float(), torch.zeros(()))
    xhk = torch.where(keep, xh, torch.zeros(()))
    return dict(dx=dx, dxs=(dx * sc).bfloat16() if b["want_scaled"] else None, dgamma=(dyk * xhk).sum(0), dbeta=dyk.sum(0))


def check_ln_bwd(out, b):
    """out: dx, dxs (or None), dgamma, dbeta (the slab partials added in fp64), colsum (third partial row, added in fp64)."""
    ref, bnd = ln_bwd_ref(b)
    keep = b["z"] != 0
    worst = {}
    for k in ("dx", "dgamma", "dbeta") + (("dxs",) if b["want_scaled"] else ()):
        got = out[k].double().cpu()
        if k in ("dgamma", "dbeta"):
            assert bool((got[~keep] == 0).all()), f"{k} is not exactly 0 in a dropped column"
        if k == "dx" and b["dres"] is not None:
            assert torch.equal(out["dx"].cpu()[:, ~keep], b["dres"][:, ~keep]), "the residual gradient does not pass through unchanged"
        if k == "dx" and b["dres"] is None:
            assert bool((got[:, ~keep] == 0).all())
        err = (got - ref[k]).abs()
        worst[k] = float((err / bnd[k].clamp_min(1e-300)).max()) if bool((bnd[k] > 0).any()) else 0.0
        assert bool((err <= bnd[k]).all()), f"{k}: {worst[k]:.2f} x its bound"
    if "colsum" in out:
        M = b["xin"].shape[0]
        want = out["dxs"].double().cpu().sum(0) if b["want_scaled"] else torch.zeros(b["xin"].shape[1], dtype=torch.float64)
        tol = gamma(M + 8) * (out["dxs"].double().cpu().abs().sum(0) if b["want_scaled"] else 0 * want)
        assert bool(((out["colsum"].double().cpu() - want).abs() <= tol).all()), "third partial row"
    return worst


# ---- b. masked operand pack ---------------------------------------------------------------------------------------------
def mask_with_zeros(n, seed, p=0.3):
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(n, generator=g)
    z[torch.rand(n, generator=g) < p] = 0
    z[0] = 0
    return z


def pack_ref(W, r, c, c_group, fault=None):
    """bf16((W * r) * c) with the products in fp32, in this order -> (rows, cols) bf16 (the transposed copy is its transpose)."""
    v = W
    if fault == "rc_swapped" and r is not None and c is not None and W.shape[0] == W.shape[1] and c_group == 1:
        r, c = c, r
    if r is not None:
        v = v * r[:, None]
    if c is not None:
        ce = c.repeat_interleave(c_group) if fault != "c_group_ignored" else c.repeat(c_group)[:W.shape[1]]
        v = v * ce[None, :]
    return v.bfloat16()


# ---- c. masked gradient finalisation --------------------------------------------------------------------------------------
def finalize_case(rows, cols, c_group, nparts, bf16, seed=0):
    g = torch.Generator().manual_seed(seed + rows + 3 * cols + nparts)
    parts = torch.randn(nparts, rows, cols, generator=g)
    return dict(parts=parts.bfloat16() if bf16 else parts, W=torch.randn(rows, cols, generator=g), r=mask_with_zeros(rows, seed + 1),
                c=mask_with_zeros(cols // c_group, seed + 2, p=0.4 if c_group == 1 else 0.0), c_group=c_group,
                dst0=torch.randn(rows, cols, generator=g), dr0=torch.randn(rows, generator=g), dc0=torch.randn(cols // c_group, generator=g))


def finalize_ref(f, overwrite, accumulate=False):
    """-> dict(dst, dr, dc) fp64 and bounds."""
    P = f["parts"].double()
    n, rows, cols = P.shape
    G, Ga = P.sum(0), P.abs().sum(0)
    e_G = gamma(n) * Ga
    r, ce = f["r"].double(), f["c"].double().repeat_interleave(f["c_group"])
    W = f["W"].double()
    rc = r[:, None] * ce[None, :]
    upd = rc * G
    dst = upd if overwrite else f["dst0"].double() + upd
    e_dst = rc.abs() * e_G + gamma(3) * upd.abs() + (0 if overwrite else U32 * dst.abs())
    t, e_t = G * W, e_G * W.abs() + U32 * (G * W).abs()
    dr = (t * ce[None, :]).sum(1)
    e_dr = (e_t * ce.abs()[None, :]).sum(1) + gamma(cols + 2) * (t * ce[None, :]).abs().sum(1)
    dck = (t * r[:, None]).sum(0)
    e_dck = (e_t * r.abs()[:, None]).sum(0) + gamma(rows + 2) * (t * r[:, None]).abs().sum(0)
    cg = f["c_group"]
    dc = dck.view(-1, cg).sum(1)
    e_dc = e_dck.view(-1, cg).sum(1) + gamma(cg) * (t * r[:, None]).abs().sum(0).view(-1, cg).sum(1)
    if accumulate:
        dr, dc = dr + f["dr0"].double(), dc + f["dc0"].double()
        e_dr, e_dc = e_dr + U32 * dr.abs(), e_dc + U32 * dc.abs()
    return dict(dst=dst, dr=dr, dc=dc), dict(dst=e_dst, dr=e_dr, dc=e_dc)


def finalize_model(f, overwrite, accumulate=False, fault=None):
    P = f["parts"].float()
    if fault == "last_part_skipped":
        P = P[:-1] if P.shape[0] > 1 else 0 * P
    G = P.sum(0)
    r, c, cg = f["r"], f["c"], f["c_group"]
    rows, cols = G.shape
    ce = c.repeat_interleave(cg) if fault != "c_group_ignored" else c.repeat(cg)[:cols]
    rr, cc = (r[:, None], ce[None, :])
    if fault == "rc_swapped":
        assert rows == cols and cg == 1
        rr, cc = ce[:, None], r[None, :]
    upd = (rr * cc) * G
    t = G * f["W"]
    dr, dc = (t * cc).sum(1), (t * rr).sum(0).view(-1, cg).sum(1)
    if accumulate:
        dr, dc = dr + f["dr0"], dc + f["dc0"]
    return dict(dst=upd if overwrite else f["dst0"] + upd, dr=dr, dc=dc)


def check_finalize(out, f, overwrite, accumulate=False):
    ref, bnd = finalize_ref(f, overwrite, accumulate)
    worst = {}
    for k in ("dst", "dr", "dc"):
        err = (out[k].double().cpu() - ref[k]).abs()
        worst[k] = float((err / bnd[k].clamp_min(1e-300)).max())
        assert bool((err <= bnd[k]).all()), f"{k}: {worst[k]:.2f} x its bound"
    z = (f["r"][:, None] * f["c"].repeat_interleave(f["c_group"])[None, :]) == 0
    if overwrite:
        assert bool((out["dst"].cpu()[z] == 0).all()), "the gradient of a masked-out weight is not exactly 0"
    return worst
