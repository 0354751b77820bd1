"""Reference, rounding model, error bound, cases and injected faults for the cascaded group attention kernel
(cream_amd/csrc/cga_attn.hip), shared by tests/test_cga_ref_cpu.py and tests/test_cga_kernel_gpu.py.

  * `head_reference` — one head in fp64, written as the model states it (EfficientViT/classification/model/efficientvit.py
    :166-178): NCHW 1 x 1 and depthwise convolutions on the windows, the literal `(q^T k) scale + ab`, softmax, `v attn^T`.
    Nothing of the kernel's indexing.
  * `kernel_model` — the whole cascade with the kernel's rounding points (feat_in, q, k, v, q', P and feat in bf16; logits,
    softmax and row sum in fp32), on the CPU, with the faults below on request.
  * `head_bound` — a per-element bound on |stored feat_i - head_reference| derived from those rounding points alone, with
    u = 2^-9 (bf16, round to nearest) and one fp32 ulp (2^-23) per accumulation step; no fitted constant.  See its docstring.
  * `check_heads` — every head of an output held against the reference of that head FED THE OUTPUT'S OWN feat_{i-1}: the stored
    bf16 value is the cascaded value by design, so every head is tested alone.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -9           # bf16 unit roundoff (round to nearest even)
ULP32 = 2.0 ** -23      # one fp32 ulp, per accumulation step: the matrix cores' internal sums are not specified to round to nearest
KEY_DIM = 16

# B, windows (rows, columns), window edge, heads, group width, kernels, layout of x
CASES = {
    "w7_h4_c16": dict(B=1, win=(1, 1), w=7, h=4, Cg=16, ks=(7, 5, 3, 3), layout="tokens"),
    "w7_h2_c48_2x2": dict(B=3, win=(2, 2), w=7, h=2, Cg=48, ks=(5, 1), layout="padded"),
    "w4_h3_c112_1x3": dict(B=1, win=(1, 3), w=4, h=3, Cg=112, ks=(7, 3, 5), layout="nchw_cl"),       # taps wider than the window
    "w8_h1_c48": dict(B=3, win=(1, 1), w=8, h=1, Cg=48, ks=(7,), layout="tokens"),
    "w1_h4_c16_2x2": dict(B=1, win=(2, 2), w=1, h=4, Cg=16, ks=(1, 3, 5, 7), layout="tokens"),
    "w7_h3_c80_1x3": dict(B=1, win=(1, 3), w=7, h=3, Cg=80, ks=(3, 5, 7), layout="nchw_cl"),
    "w8_h4_c112_2x2": dict(B=3, win=(2, 2), w=8, h=4, Cg=112, ks=(7, 5, 3, 1), layout="padded"),
    "w5_h2_c16": dict(B=1, win=(1, 3), w=5, h=2, Cg=16, ks=(5, 3), layout="tokens"),                 # N = 25: two token tiles
    "w6_h2_c32": dict(B=1, win=(2, 2), w=6, h=2, Cg=32, ks=(3, 7), layout="padded"),                 # N = 36: three token tiles
}

FAULTS = ("taps_transposed", "pad_read_through", "ab_prev_head", "wrong_chunk", "pad_rows_in_softmax")


def make_case(c, seed=0):
    """-> (x (B, Hs, Ws, C) bf16 in the case's layout, ops): ops = dict(W, b, taps, tb: per-head lists of fp32 tensors, the
    weights already bf16 values; ab (h, N, N) fp32; scale)."""
    g = torch.Generator().manual_seed(1000 + seed)
    B, (ny, nx), w, h, Cg = c["B"], c["win"], c["w"], c["h"], c["Cg"]
    Hs, Ws, C, N = ny * w, nx * w, h * Cg, w * w
    r = lambda *s: torch.randn(*s, generator=g)                    # noqa: E731
    x = r(B, Hs, Ws, C).bfloat16()
    if c["layout"] == "padded":                                    # a slice of a larger buffer: every stride is its own
        buf = torch.zeros(B, Hs + 1, Ws + 2, C + 8, dtype=torch.bfloat16)
        buf[:, :Hs, :Ws, :C] = x
        x = buf[:, :Hs, :Ws, :C]
    elif c["layout"] == "nchw_cl":                                 # a channels-last NCHW tensor, seen as (B, H, W, C)
        x = x.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    ops = dict(W=[(r(32 + Cg, Cg) / Cg ** 0.5).bfloat16().float() for _ in range(h)], b=[0.1 * r(32 + Cg) for _ in range(h)],
               taps=[r(KEY_DIM, k, k) / k for k in c["ks"]], tb=[0.1 * r(KEY_DIM) for _ in range(h)],
               ab=0.5 * r(h, N, N), scale=KEY_DIM ** -0.5)
    return x, ops


def to_pack(ops, device):
    from cream_amd import cga_attn
    mv = lambda ts: [t.to(device) for t in ts]                     # noqa: E731
    return cga_attn.pack_operands(mv(ops["W"]), mv(ops["b"]), mv(ops["taps"]), mv(ops["tb"]), ops["ab"].to(device))


def partition(t, w):
    """(B, Hs, Ws, C) -> (windows, w^2, C)."""
    B, Hs, Ws, C = t.shape
    return t.reshape(B, Hs // w, w, Ws // w, w, C).transpose(2, 3).reshape(-1, w * w, C)


def reverse(t, w, B, Hs, Ws):
    """(windows, w^2, C) -> (B, Hs, Ws, C)."""
    return t.reshape(B, Hs // w, Ws // w, w, w, -1).transpose(2, 3).reshape(B, Hs, Ws, -1)


# ---- the reference: one head, as the model states it ------------------------------------------------------------------------------
def head_reference(feat_in, i, ops, w):
    """feat_in (B, Hs, Ws, Cg) fp64, the exact input of head i -> feat_i (B, Hs, Ws, Cg) fp64."""
    B, Hs, Ws, Cg = feat_in.shape
    d = lambda t: t.double()                                       # noqa: E731
    k_i = ops["taps"][i].shape[-1]
    xw = partition(feat_in, w).transpose(1, 2).reshape(-1, Cg, w, w)                       # (windows, Cg, w, w): NCHW
    feat = F.conv2d(xw, d(ops["W"][i])[:, :, None, None], d(ops["b"][i]))
    q, k, v = feat.split([KEY_DIM, KEY_DIM, Cg], dim=1)
    q = F.conv2d(q, d(ops["taps"][i])[:, None], d(ops["tb"][i]), padding=k_i // 2, groups=KEY_DIM)
    q, k, v = q.flatten(2), k.flatten(2), v.flatten(2)
    attn = (q.transpose(-2, -1) @ k) * ops["scale"] + d(ops["ab"][i])
    attn = attn.softmax(dim=-1)
    feat = v @ attn.transpose(-2, -1)                                                      # (windows, Cg, N)
    return reverse(feat.transpose(1, 2), w, B, Hs, Ws)


# ---- the depthwise convolution inside a window as a matrix ---------------------------------------------------------------------------
def conv_matrix(taps, w):
    """taps (16, k, k) -> T (16, N, N) fp64 with q'[n, c] = sum_m T[c, n, m] q[m, c]: zero padding inside the window."""
    k = taps.shape[-1]
    R, N = k // 2, w * w
    T = torch.zeros(KEY_DIM, N, N, dtype=torch.float64)
    for y in range(w):
        for x in range(w):
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    if 0 <= y + dy < w and 0 <= x + dx < w:
                        T[:, y * w + x, (y + dy) * w + x + dx] = taps[:, dy + R, dx + R].double()
    return T


# ---- the bound ----------------------------------------------------------------------------------------------------------------------
def head_bound(prev, xi, i, ops, w):
    """prev = stored feat_{i-1} (None for head 0), xi = x's group i, both (B, Hs, Ws, Cg) -> bound (B, Hs, Ws, Cg) fp64 on
    |stored feat_i - head_reference(prev + xi)|.

    Every rounding point contributes its unit roundoff times the magnitude of what it rounds, carried forward through the
    absolute values of the linear maps; second-order products are kept, so nothing is dropped:
      feat_in  u |prev + xi| (head 0 copies x: 0)
      q, k, v  |W| e_in + (K + 2) ulp32 (|W| |feat_in| + |b|), then u of the value for the bf16 store
      q'       |T| e_q + (k^2 + 2) ulp32 (|T| |q| + |tb|), then u
      logits   scale (e_q' |k| + |q'| e_k + e_q' e_k) + 18 ulp32 (scale |q'| |k| + |ab|) + the exponential's own error as an
               error of its argument, (2 + |l - max|) ulp32 (one rounding of the difference, the argument's scaling to base 2,
               one ulp of the hardware exponential)
      softmax  p~_m / p_m = e^{d_m} / sum_j p_j e^{d_j} with |d_j| <= e_j lies in [e^{-e_m} / sum_j p_j e^{e_j},
               e^{e_m} / sum_j p_j e^{-e_j}] — exact, not linearised
      feat     |dP| |v| + P e_v + u P |v| (P enters the product as bf16) + (N + 4) ulp32 P |v| (the product's and the row sum's
               accumulation, the division), then u for the bf16 store."""
    d = lambda t: t.double()                                       # noqa: E731
    B, Hs, Ws, Cg = xi.shape
    N = w * w
    xs = partition(d(xi), w)
    if prev is None:
        s, e_in = xs, torch.zeros_like(xs)
    else:
        s = partition(d(prev), w) + xs
        e_in = (U + ULP32) * s.abs()
    W, b = d(ops["W"][i]), d(ops["b"][i])
    y = s @ W.T + b
    e_pre = e_in @ W.abs().T + (Cg + 32 + 2) * ULP32 * ((s.abs() + e_in) @ W.abs().T + b.abs())
    e_y = e_pre + U * (y.abs() + e_pre)
    q, k, v = y.split([KEY_DIM, KEY_DIM, Cg], dim=-1)
    e_q, e_k, e_v = e_y.split([KEY_DIM, KEY_DIM, Cg], dim=-1)
    T, tb = conv_matrix(ops["taps"][i], w), d(ops["tb"][i])
    kk = ops["taps"][i].shape[-1] ** 2
    qc = torch.einsum("cnm,wmc->wnc", T, q) + tb
    e_pre = torch.einsum("cnm,wmc->wnc", T.abs(), e_q) + (kk + 2) * ULP32 * (torch.einsum("cnm,wmc->wnc", T.abs(), q.abs() + e_q) + tb.abs())
    e_qc = e_pre + U * (qc.abs() + e_pre)
    sc, ab = ops["scale"], d(ops["ab"][i])
    kt = k.transpose(1, 2)
    l = sc * (qc @ kt) + ab
    e_l = sc * (e_qc @ kt.abs() + qc.abs() @ e_k.transpose(1, 2) + e_qc @ e_k.transpose(1, 2))
    e_l = e_l + 18 * ULP32 * (sc * ((qc.abs() + e_qc) @ (kt.abs() + e_k.transpose(1, 2))) + ab.abs())
    e_l = e_l + (2 + (l - l.max(-1, keepdim=True).values).abs() + 2 * e_l) * ULP32
    p = l.softmax(-1)
    lo = (-e_l).exp() / (p * e_l.exp()).sum(-1, keepdim=True)
    hi = e_l.exp() / (p * (-e_l).exp()).sum(-1, keepdim=True)
    dp = p * torch.maximum(hi - 1, 1 - lo)
    f = p @ v
    pv = (p + dp) @ (v.abs() + e_v)
    e_pre = dp @ v.abs() + (p + dp) @ e_v + U * pv + (N + 4) * ULP32 * pv
    e_f = e_pre + U * (f.abs() + e_pre)
    return reverse(e_f, w, B, Hs, Ws) + 1e-30


# ---- the kernel's arithmetic, on the CPU ----------------------------------------------------------------------------------------------
def _whole_map_conv(q, taps, tb, w, B, Hs, Ws):
    """The fault: the depthwise convolution on the whole map, so that a window's border reads its neighbour."""
    k = taps.shape[-1]
    qm = reverse(q, w, B, Hs, Ws).permute(0, 3, 1, 2)
    out = F.conv2d(qm, taps[:, None], tb, padding=k // 2, groups=KEY_DIM)
    return partition(out.permute(0, 2, 3, 1), w)


def kernel_model(x, ops, w, fault=None):
    """x (B, Hs, Ws, C) bf16 -> the stored pre-ReLU output (B, Hs, Ws, C) bf16, with the kernel's rounding points.  `fault`: one
    of FAULTS, a wrong kernel that the bound has to catch."""
    assert fault is None or fault in FAULTS
    B, Hs, Ws, C = x.shape
    h, N = len(ops["W"]), w * w
    Cg = C // h
    bf = lambda t: t.bfloat16().float()                            # noqa: E731
    xs = partition(x.float(), w)                                   # (windows, N, C)
    NP = (N + 15) // 16 * 16
    outs, feat = [], None
    for i in range(h):
        chunk = (i + 1) % h if (fault == "wrong_chunk" and i > 0) else i
        xi = xs[..., chunk * Cg:(chunk + 1) * Cg]
        fin = xi if feat is None else bf(feat + xi)
        y = bf(fin @ ops["W"][i].T + ops["b"][i])
        q, k, v = y.split([KEY_DIM, KEY_DIM, Cg], dim=-1)
        taps = ops["taps"][i].transpose(-1, -2) if fault == "taps_transposed" else ops["taps"][i]
        if fault == "pad_read_through":
            qc = bf(_whole_map_conv(q, taps, ops["tb"][i], w, B, Hs, Ws))
        else:
            qc = bf(torch.einsum("cnm,wmc->wnc", conv_matrix(taps, w).float(), q) + ops["tb"][i])
        ab = ops["ab"][(i - 1) % h if fault == "ab_prev_head" else i]
        l = ops["scale"] * (qc @ k.transpose(1, 2)) + ab
        if fault == "pad_rows_in_softmax" and NP > N:
            # the pad tokens of the tile: zero input rows, so k and v are their biases; no attention bias
            pad = bf(ops["b"][i]).expand(l.shape[0], NP - N, -1)
            l = torch.cat([l, ops["scale"] * (qc @ pad[..., KEY_DIM:2 * KEY_DIM].transpose(1, 2))], -1)
            v = torch.cat([v, pad[..., 2 * KEY_DIM:]], 1)
        p = (l - l.max(-1, keepdim=True).values).exp()
        feat = bf((bf(p) @ v) / p.sum(-1, keepdim=True))
        outs.append(feat)
    return reverse(torch.cat(outs, -1), w, B, Hs, Ws).bfloat16()


# ---- every head of an output, alone ------------------------------------------------------------------------------------------------------
def check_heads(out, x, ops, w):
    """out (B, Hs, Ws, C): a stored pre-ReLU output for x -> [(head, worst |error| / bound, worst |error|)].  Head i's reference
    is fed the output's own feat_{i-1}."""
    h = len(ops["W"])
    Cg = x.shape[-1] // h
    out, x = out.detach().cpu().double(), x.detach().cpu().double()
    res = []
    for i in range(h):
        xi = x[..., i * Cg:(i + 1) * Cg]
        prev = out[..., (i - 1) * Cg:i * Cg] if i else None
        ref = head_reference(xi if prev is None else prev + xi, i, ops, w)
        err = (out[..., i * Cg:(i + 1) * Cg] - ref).abs()
        res.append((i, float((err / head_bound(prev, xi, i, ops, w)).max()), float(err.max())))
    return res
