"""Reference, rounding model, error bound, cases and injected faults for the depthwise 3 x 3 + FFN kernel and the proj +
residual kernel (cream_amd/csrc/evit_ffn.hip), shared by tests/test_evit_ffn_ref_cpu.py and tests/test_evit_ffn_kernel_gpu.py.

  * `reference` — the pair in fp64, written as the model states it (EfficientViT/classification/model/efficientvit.py:78-101,
    :263-282): `F.conv2d` on NCHW with `groups=C`, then pw1 -> ReLU -> pw2, and `x + m(x)` twice.  Nothing of the kernel's
    indexing.  `pw_reference` likewise: res + conv1x1(a).
  * `kernel_model` — the kernel's rounding points on the CPU (x bf16; taps, bias and y1 fp32; the first product reads bf16(y1);
    hidden = bf16(relu(fp32 + b1)); the second product fp32 on top of the fp32 y1; out = bf16(.. + b2)), with the faults below
    on request.
  * `bound` — a per-element bound on |out - reference| derived from those rounding points alone, with u = 2^-9 (bf16, round to
    nearest) and one fp32 ulp (2^-23) per product and per accumulation step; no fitted constant.  See its docstring.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -9           # bf16, round to nearest even: half an ulp of a value in [1, 2); see `rnd`
ULP32 = 2.0 ** -23      # one fp32 ulp per step: the matrix cores' internal sums are not specified to round to nearest
HC = 64                 # the kernel's hidden chunk (the `b1_per_chunk` fault needs it)

CASES = {
    "a_c64_14x14": dict(C=64, Ch=128, H=14, W=14, B=1, layout="tokens"),        # row strips and halo rows inside one image
    "b_c192_14x14": dict(C=192, Ch=384, H=14, W=14, B=2, layout="padded"),      # a halo at an image boundary; padding never read
    "c_c144_7x7": dict(C=144, Ch=288, H=7, W=7, B=3, layout="nchw_cl"),         # K tail 144 = 4.5 x 32; 49 of 64 tokens
    "d_c384_4x4": dict(C=384, Ch=768, H=4, W=4, B=5, layout="tokens"),          # four images per tile, ragged last tile, 12 chunks
    "e_c16_1x1": dict(C=16, Ch=32, H=1, W=1, B=2, layout="tokens"),             # every tap but the centre is padding
    "f_c224_10x10": dict(C=224, Ch=448, H=10, W=10, B=1, layout="padded"),      # the padded recipe's map
    "g_c32_3x5": dict(C=32, Ch=64, H=3, W=5, B=2, layout="nchw_cl"),            # H != W
    "h_c240_5x5": dict(C=240, Ch=480, H=5, W=5, B=4, layout="tokens"),          # second K tail; images straddling tiles
}
# the grid is one workgroup per 64 tokens, never persistent: there is no looping case to force

FAULTS = ("halo_wraps_row", "halo_wraps_image", "taps_transposed", "residual_from_x", "no_relu", "k_tail_read_through",
          "b1_per_chunk")

LAYOUTS = ("tokens", "padded", "nchw_cl")

# (Cin, Cout), map, B, layout of a, layout of res
PW_CASES = {
    "pw_64_64_7x7": dict(Cin=64, Cout=64, H=7, W=7, B=3, la="tokens", lr="nchw_cl"),
    "pw_144_144_4x4": dict(Cin=144, Cout=144, H=4, W=4, B=5, la="padded", lr="tokens"),
    "pw_384_384_7x7": dict(Cin=384, Cout=384, H=7, W=7, B=2, la="nchw_cl", lr="padded"),
    "pw_96_64_4x4": dict(Cin=96, Cout=64, H=4, W=4, B=3, la="tokens", lr="padded"),
    "pw_64_64_4x4": dict(Cin=64, Cout=64, H=4, W=4, B=1, la="padded", lr="nchw_cl"),
    "pw_96_64_7x7": dict(Cin=96, Cout=64, H=7, W=7, B=1, la="nchw_cl", lr="tokens"),
}

PAD_VALUE = 64.0        # what a padded buffer holds outside the slice: a kernel that reads it leaves the bound at once


def in_layout(x, layout):
    """x (B, H, W, C) bf16 contiguous -> the same values in `layout`."""
    B, H, W, C = x.shape
    if layout == "padded":                                         # a slice of a larger buffer: every stride is its own
        buf = torch.full((B, H + 1, W + 2, C + 8), PAD_VALUE, dtype=torch.bfloat16)
        buf[:, :H, :W, :C] = x
        return buf[:, :H, :W, :C]
    if layout == "nchw_cl":                                        # a channels-last NCHW tensor, seen as (B, H, W, C)
        return x.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    assert layout == "tokens"
    return x


def to_device(x, device, layout):
    """Keeps a slice a slice (and every stride) on the device."""
    xd = x._base.to(device)[:, :x.shape[1], :x.shape[2], :x.shape[3]] if layout == "padded" else x.to(device)
    assert xd.stride() == x.stride() and xd.is_contiguous() == (layout == "tokens" or x.is_contiguous()), (xd.stride(), x.stride())
    return xd


def make_case(c, seed=0, layout=None):
    """-> (x (B, H, W, C) bf16 in the case's layout, ops): ops = dict(taps (C, 3, 3), dwb (C), w1 (Ch, C), b1 (Ch), w2 (C, Ch),
    b2 (C)), fp32, the 1 x 1 weights already bf16 values."""
    g = torch.Generator().manual_seed(2000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)                    # noqa: E731
    C, Ch = c["C"], c["Ch"]
    x = r(c["B"], c["H"], c["W"], C).bfloat16()
    ops = dict(taps=r(C, 3, 3) / 3, dwb=0.1 * r(C), w1=(r(Ch, C) / C ** 0.5).bfloat16().float(), b1=0.1 * r(Ch),
               w2=(r(C, Ch) / Ch ** 0.5).bfloat16().float(), b2=0.1 * r(C))
    return in_layout(x, layout or c["layout"]), ops


def make_pw_case(c, seed=0):
    """-> (a, res, ops): ops = dict(w (Cout, Cin) bf16 values, b (Cout))."""
    g = torch.Generator().manual_seed(3000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)                    # noqa: E731
    a = torch.relu(r(c["B"], c["H"], c["W"], c["Cin"])).bfloat16()                 # the attention's output comes through a ReLU
    res = r(c["B"], c["H"], c["W"], c["Cout"]).bfloat16()
    ops = dict(w=(r(c["Cout"], c["Cin"]) / c["Cin"] ** 0.5).bfloat16().float(), b=0.1 * r(c["Cout"]))
    return in_layout(a, c["la"]), in_layout(res, c["lr"]), ops


def to_pack(ops, device):
    from cream_amd import evit_ffn
    return evit_ffn.pack_dwffn(*(ops[n].to(device) for n in ("taps", "dwb", "w1", "b1", "w2", "b2")))


def to_pw_pack(ops, device):
    from cream_amd import evit_ffn
    return evit_ffn.pack_pw(ops["w"].to(device), ops["b"].to(device))


# ---- the references: as the model states them ---------------------------------------------------------------------------------
def _parts(x, ops):
    """-> (y1, h, y2) fp64 NCHW: the first Residual's output, the FFN's hidden activation after the ReLU, the output."""
    d = lambda t: t.double()                                       # noqa: E731
    xn = d(x).permute(0, 3, 1, 2)
    C = xn.shape[1]
    y1 = xn + F.conv2d(xn, d(ops["taps"])[:, None], d(ops["dwb"]), padding=1, groups=C)
    h = F.relu(F.conv2d(y1, d(ops["w1"])[:, :, None, None], d(ops["b1"])))
    y2 = y1 + F.conv2d(h, d(ops["w2"])[:, :, None, None], d(ops["b2"]))
    return y1, h, y2


def reference(x, ops):
    """x (B, H, W, C) -> (B, H, W, C) fp64."""
    return _parts(x, ops)[2].permute(0, 2, 3, 1)


def pw_reference(a, res, ops):
    d = lambda t: t.double()                                       # noqa: E731
    y = d(res).permute(0, 3, 1, 2) + F.conv2d(d(a).permute(0, 3, 1, 2), d(ops["w"])[:, :, None, None], d(ops["b"]))
    return y.permute(0, 2, 3, 1)


# ---- the bounds -------------------------------------------------------------------------------------------------------------------
def rnd(m):
    """What one rounding to bf16 costs a value of magnitude at most m: half an ulp, u 2^(floor(log2 m) + 1) with u = 2^-9 — u |v|
    only for a value just below a power of two, 2 u |v| just above one (4.0155 rounds to 4, an error of 2^-8.01 of the value)."""
    return U * torch.exp2(torch.floor(torch.log2(m.clamp_min(2.0 ** -126))) + 1)


def bound(x, ops):
    """x (B, H, W, C) -> bound (B, H, W, C) fp64 on |out - reference|.

    Every rounding point contributes its unit roundoff times the magnitude of what it rounds, carried forward through the
    absolute values of the linear maps; second-order products are kept:
      y1      x is exact.  Nine products and nine additions, the bias and the residual, each one fp32 rounding of a partial sum
              that |x| + |taps| * |x| + |dwb| bounds:  e_1 = 20 ulp32 (|x| + |taps| * |x| + |dwb|)
      operand bf16(y1):  e_a = e_1 + rnd(|y1| + e_1), half a bf16 ulp at that magnitude (`rnd`)
      hidden  |W1| e_a + (KP + 2) ulp32 (|W1| (|y1| + e_a) + |b1|) with KP = C rounded up to 32 accumulation steps, the bias
              and the ReLU (1-Lipschitz), then rnd of the value for the bf16 store
      out     the fp32 y1 starts the accumulator: e_1 + |W2| e_h + (Ch + 3) ulp32 (|y1| + e_1 + |W2| (h + e_h) + |b2|), then rnd
              of the value for the bf16 store."""
    d = lambda t: t.double()                                       # noqa: E731
    y1, h, y2 = _parts(x, ops)
    C, Ch = ops["w2"].shape
    xa = d(x).permute(0, 3, 1, 2).abs()
    e1 = 20 * ULP32 * (xa + F.conv2d(xa, d(ops["taps"]).abs()[:, None], d(ops["dwb"]).abs(), padding=1, groups=C))
    ea = e1 + rnd(y1.abs() + e1)
    w1a, w2a = d(ops["w1"]).abs()[:, :, None, None], d(ops["w2"]).abs()[:, :, None, None]
    KP = (C + 31) // 32 * 32
    ehp = F.conv2d(ea, w1a) + (KP + 2) * ULP32 * F.conv2d(y1.abs() + ea, w1a, d(ops["b1"]).abs())
    eh = ehp + rnd(h + ehp)
    eo = e1 + F.conv2d(eh, w2a) + (Ch + 3) * ULP32 * (y1.abs() + e1 + F.conv2d(h + eh, w2a, d(ops["b2"]).abs()))
    return (eo + rnd(y2.abs() + eo)).permute(0, 2, 3, 1) + 1e-30


def pw_bound(a, res, ops):
    """|out - pw_reference|: a, res and W are exact; KP accumulation steps, the bias and the residual in fp32, then the bf16
    store:  e = (KP + 3) ulp32 (|res| + |W| |a| + |b|),  bound = e + rnd(|ref| + e)."""
    d = lambda t: t.double()                                       # noqa: E731
    Cin = ops["w"].shape[1]
    KP = (Cin + 31) // 32 * 32
    mag = d(res).permute(0, 3, 1, 2).abs() + F.conv2d(d(a).permute(0, 3, 1, 2).abs(), d(ops["w"]).abs()[:, :, None, None],
                                                      d(ops["b"]).abs())
    e = (KP + 3) * ULP32 * mag.permute(0, 2, 3, 1)
    return e + rnd(pw_reference(a, res, ops).abs() + e) + 1e-30


# ---- the kernel's arithmetic, on the CPU ------------------------------------------------------------------------------------------
def _flat_dw(xf, taps, halo=None):
    """The depthwise sum on the flat token axis, tap after tap in fp32: (B, H, W, C) fp32 -> the nine-tap sum with the neighbour
    of token n taken at n + dy W + dx where it lies inside the token's own map.  The faults: `halo` = "row" checks the image
    only, so a row's end wraps into the next row; "image" checks the column but not the row, so the first and last rows read
    the neighbouring image."""
    B, H, W, C = xf.shape
    flat = xf.reshape(B * H * W, C)
    n = torch.arange(B * H * W)
    img, row, col = n // (H * W), n // W % H, n % W
    out = torch.zeros_like(flat)
    for ky in range(3):
        for kx in range(3):
            m = n + (ky - 1) * W + kx - 1
            inside_row = (col + kx - 1 >= 0) & (col + kx - 1 < W)
            if halo == "image":
                ok = (m >= 0) & (m < B * H * W) & inside_row
            elif halo == "row":
                ok = (m >= img * H * W) & (m < (img + 1) * H * W)
            else:
                ok = (row + ky - 1 >= 0) & (row + ky - 1 < H) & inside_row
            out += torch.where(ok[:, None], flat[m.clamp(0, B * H * W - 1)] * taps[:, ky, kx], torch.zeros(()))
    return out.reshape(B, H, W, C)


def kernel_model(x, ops, fault=None):
    """x (B, H, W, C) bf16 -> (B, H, W, C) bf16 with the kernel's rounding points.  `fault`: one of FAULTS, a wrong kernel that
    the bound has to catch."""
    assert fault is None or fault in FAULTS
    bf = lambda t: t.bfloat16().float()                            # noqa: E731
    B, H, W, C = x.shape
    Ch = ops["w1"].shape[0]
    xf = x.float()
    taps = ops["taps"].transpose(-1, -2) if fault == "taps_transposed" else ops["taps"]
    s = _flat_dw(xf, taps, {"halo_wraps_row": "row", "halo_wraps_image": "image"}.get(fault))
    y1 = xf + (s + ops["dwb"])                                     # fp32
    a = bf(y1).reshape(-1, C)
    acc = a @ ops["w1"].T
    KP = (C + 31) // 32 * 32
    if fault == "k_tail_read_through" and KP > C:
        # the operand rows are read KP wide at a pitch of C: the tail columns are the next row's first ones
        a_next = torch.cat([a[1:], a[-1:]])[:, :KP - C]
        w_next = torch.cat([ops["w1"][1:], ops["w1"][-1:]])[:, :KP - C]
        acc = acc + a_next @ w_next.T
    nb1 = (Ch + HC - 1) // HC if fault == "b1_per_chunk" else 1
    hid = acc + nb1 * ops["b1"]
    hid = bf(hid if fault == "no_relu" else torch.relu(hid))
    base = xf if fault == "residual_from_x" else y1
    out = base.reshape(-1, C) + hid @ ops["w2"].T + ops["b2"]
    return out.reshape(B, H, W, C).bfloat16()


def pw_kernel_model(a, res, ops):
    """The proj kernel's rounding points: fp32(res) + b + fp32 products, one rounding to bf16."""
    out = res.float() + ops["b"] + (a.float().reshape(-1, a.shape[-1]) @ ops["w"].T).reshape(res.shape)
    return out.bfloat16()


def worst(out, ref, bnd):
    """-> (worst |error| / bound, worst |error|)."""
    err = (out.detach().cpu().double() - ref).abs()
    return float((err / bnd).max()), float(err.max())
