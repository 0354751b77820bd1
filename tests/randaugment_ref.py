"""Test support: a numpy restatement of the 15 RandAugment operations as the device applies them (csrc/image_augment.hip), one
descriptor (cream_amd.autoformer.data.AugDesc) at a time, on (H, W, 3) uint8 images.  Every op is Pillow's on a uint8 RGB image,
restated integer for integer (the affine op in doubles, in libImaging's order of operations); tests/test_randaugment_cpu.py pins it
against the installed Pillow and the committed Pillow-made fixtures, the GPU tests pin the device against it (Pillow may be
missing there).
    AutoContrast / Equalize   ImageOps.autocontrast (cutoff 0) / ImageOps.equalize: per-channel histogram -> 256-entry LUT
    Invert / Posterize / Solarize / SolarizeAdd   the LUTs of ImageOps.invert / posterize / solarize and timm's solarize_add
    Color / Contrast / Brightness / Sharpness     ImageEnhance: Image.blend(degenerate, image, float32(factor))
    affine (Rotate, Shear*, Translate*Rel)        Image.transform(size, AFFINE, m, BICUBIC, fillcolor) = libImaging/Geometry.c
"""
import numpy as np

from cream_amd.autoformer import data as D


def grey(img):
    """RGB -> L of libImaging/Convert.c: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    i = img.astype(np.int64)
    return ((19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, img, factor):
    """Image.blend(degenerate, img, alpha) of libImaging/Blend.c: float32 in1 + alpha * (in2 - in1), clipped, truncated."""
    a = np.float32(factor)
    d = degenerate.astype(np.int32)
    t = d.astype(np.float32) + a * (img.astype(np.int32) - d).astype(np.float32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.uint8)


def _lut(img, luts):
    return np.stack([luts[c][img[..., c]] for c in range(3)], axis=-1).astype(np.uint8)


def autocontrast_lut(channel):
    h = np.bincount(channel.reshape(-1), minlength=256)
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(ix * scale + offset))) for ix in range(256)])


def equalize_lut(channel):
    h = np.bincount(channel.reshape(-1), minlength=256)
    nz = h[h > 0]
    if len(nz) <= 1:
        return np.arange(256)
    step = (int(nz.sum()) - int(nz[-1])) // 255
    if step == 0:
        return np.arange(256)
    n = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum(n // step, 255)


def smooth(img):
    """ImageFilter.SMOOTH (3 x 3 kernel 1 1 1 / 1 5 1 / 1 1 1, scale 13): the border rows and columns copied, the interior
    rounded to nearest."""
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    i = img.astype(np.int64)
    acc = 4 * i[1:-1, 1:-1]
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            acc = acc + i[dy:dy + H - 2, dx:dx + W - 2]
    out[1:-1, 1:-1] = ((acc + 6) // 13).astype(np.uint8)
    return out


def _cubic(v1, v2, v3, v4, d):
    """libImaging/Geometry.c BICUBIC, in its order of operations (integer taps: the p's are exact; double taps: IEEE doubles)."""
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, m, fill):
    """Image.transform(size, AFFINE, m, BICUBIC, fillcolor=fill): per output pixel the input point (a (x + .5) + b (y + .5) + c,
    ...) in doubles; outside [0, W) x [0, H) the fill colour, else the 4 x 4 bicubic taps around it (clamped to the image),
    along x per row, then along y; 0 / 255 at the ends, truncated between."""
    H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    xo, yo = xx + 0.5, yy + 0.5
    xin = m[0] * xo + m[1] * yo + m[2]
    yin = m[3] * xo + m[4] * yo + m[5]
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = xin - x, yin - y
    cols = [np.clip(x - 1 + k, 0, W - 1) for k in range(4)]
    rows = [np.clip(y - 1 + k, 0, H - 1) for k in range(4)]
    src = img.astype(np.int64)
    out = np.empty_like(img)
    for c in range(3):
        v = [_cubic(*[src[r, cc, c] for cc in cols], dx) for r in rows]
        v = _cubic(v[0], v[1], v[2], v[3], dy)
        o = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, np.trunc(np.clip(v, 0, 255))))
        out[..., c] = np.where(inside, o, fill[c]).astype(np.uint8)
    return out


def apply(img, op):
    """One AugDesc on an (H, W, 3) uint8 image."""
    kind, arg, factor, fill, m = op
    i = np.arange(256)
    if kind == D.AUG_NONE:
        return img.copy()
    if kind == D.AUG_AUTOCONTRAST:
        return _lut(img, [autocontrast_lut(img[..., c]) for c in range(3)])
    if kind == D.AUG_EQUALIZE:
        return _lut(img, [equalize_lut(img[..., c]) for c in range(3)])
    if kind == D.AUG_INVERT:
        return (255 - img).astype(np.uint8)
    if kind == D.AUG_POSTERIZE:
        return (img & np.uint8(~(2 ** (8 - arg) - 1) & 255)).astype(np.uint8)
    if kind == D.AUG_SOLARIZE:
        return _lut(img, [np.where(i < arg, i, 255 - i)] * 3)
    if kind == D.AUG_SOLARIZE_ADD:
        return _lut(img, [np.where(i < 128, np.minimum(255, i + arg), i)] * 3)
    if kind == D.AUG_COLOR:
        return blend(np.repeat(grey(img)[..., None], 3, axis=-1), img, factor)
    if kind == D.AUG_CONTRAST:
        h = np.bincount(grey(img).reshape(-1), minlength=256)
        mean = int(int((np.arange(256) * h).sum()) / (img.shape[0] * img.shape[1]) + 0.5)      # ImageStat's mean, in doubles
        return blend(np.full_like(img, mean), img, factor)
    if kind == D.AUG_BRIGHTNESS:
        return blend(np.zeros_like(img), img, factor)
    if kind == D.AUG_SHARPNESS:
        return blend(smooth(img), img, factor)
    if kind == D.AUG_AFFINE:
        return affine(img, m, fill)
    raise ValueError(f"unknown op kind {kind}")


def apply_chain(img, ops):
    for op in ops:
        img = apply(img, op)
    return img
