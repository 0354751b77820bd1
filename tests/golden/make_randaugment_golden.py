"""Golden vectors of the RandAugment operations, made with the library timm's RandAugment calls: Pillow.
    python tests/golden/make_randaugment_golden.py        ->  tests/golden/randaugment.npz
Seeded uint8 RGB images (1 x 1, 2 x 3, odd sizes and one 224 x 224 one of constant blocks) and, for every op kind at extreme and typical
arguments, the descriptor (cream_amd.autoformer.data.AugDesc) and what Pillow's own call gives:
    ImageOps.autocontrast / equalize / invert / posterize / solarize, timm's solarize_add (Image.point),
    ImageEnhance.Color / Contrast / Brightness / Sharpness(img).enhance(factor),
    img.rotate(deg, resample=BICUBIC, fillcolor=fill), img.transform(size, AFFINE, m, BICUBIC, fillcolor=fill).
Pillow version used is recorded in the file."""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from cream_amd.autoformer import data as D  # noqa: E402

FILL = (124, 116, 104)


def images():
    rng = np.random.default_rng(20261016)
    out = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((1, 1), (2, 3), (5, 7), (13, 17))]
    out.append(rng.integers(100, 150, (9, 11, 3), dtype=np.uint8))                 # low contrast
    blocks = rng.integers(20, 236, (8, 8, 3), dtype=np.uint8)                     # 224 x 224 of 28 x 28 blocks (compresses)
    out.append(np.ascontiguousarray(np.repeat(np.repeat(blocks, 28, axis=0), 28, axis=1)))
    return out


def pillow(img, op, deg=None):
    im = Image.fromarray(img)
    kind, arg, factor, fill, m = op
    if deg is not None:
        return im.rotate(deg, resample=Image.BICUBIC, fillcolor=fill)
    if kind == D.AUG_AUTOCONTRAST:
        return ImageOps.autocontrast(im)
    if kind == D.AUG_EQUALIZE:
        return ImageOps.equalize(im)
    if kind == D.AUG_INVERT:
        return ImageOps.invert(im)
    if kind == D.AUG_POSTERIZE:
        return ImageOps.posterize(im, arg)
    if kind == D.AUG_SOLARIZE:
        return ImageOps.solarize(im, arg)
    if kind == D.AUG_SOLARIZE_ADD:
        return im.point([min(255, i + arg) if i < 128 else i for i in range(256)] * 3)
    if kind in (D.AUG_COLOR, D.AUG_CONTRAST, D.AUG_BRIGHTNESS, D.AUG_SHARPNESS):
        cls = {D.AUG_COLOR: ImageEnhance.Color, D.AUG_CONTRAST: ImageEnhance.Contrast, D.AUG_BRIGHTNESS: ImageEnhance.Brightness,
               D.AUG_SHARPNESS: ImageEnhance.Sharpness}[kind]
        return cls(im).enhance(factor)
    if kind == D.AUG_AFFINE:
        return im.transform(im.size, Image.AFFINE, m, Image.BICUBIC, fillcolor=fill)
    return im.copy()


def cases(h, w, big):
    """(descriptor, rotate degrees or None) per case; the 224 x 224 image: a few of them (size of the file)."""
    if big:
        return [(D.AugDesc(D.AUG_EQUALIZE), None), (D.AugDesc(D.AUG_AUTOCONTRAST), None),
                (D.AugDesc(D.AUG_SHARPNESS, factor=1.81), None), (D.AugDesc(D.AUG_CONTRAST, factor=0.19), None),
                (D.AugDesc(D.AUG_AFFINE, fill=FILL, m=D._rotate_matrix(27.0, w, h)), 27.0),
                (D.AugDesc(D.AUG_AFFINE, fill=FILL, m=D._rotate_matrix(-30.0, w, h)), -30.0),
                (D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, 0.27, 0, 0, 1, 0)), None),
                (D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, 0, 0, 0, 1, -0.45 * h)), None)]
    out = [(D.AugDesc(D.AUG_NONE), None), (D.AugDesc(D.AUG_AUTOCONTRAST), None), (D.AugDesc(D.AUG_EQUALIZE), None),
           (D.AugDesc(D.AUG_INVERT), None)]
    out += [(D.AugDesc(D.AUG_POSTERIZE, arg=b), None) for b in ((0, 4) if big else (0, 1, 4, 8))]
    out += [(D.AugDesc(D.AUG_SOLARIZE, arg=t), None) for t in ((26, 256) if big else (0, 26, 128, 256))]
    out += [(D.AugDesc(D.AUG_SOLARIZE_ADD, arg=a), None) for a in ((99,) if big else (0, 99, 110))]
    factors = (0.19, 1.81) if big else (0.1, 0.19, 1.0, 1.81, 1.9)
    for kind in (D.AUG_COLOR, D.AUG_CONTRAST, D.AUG_BRIGHTNESS, D.AUG_SHARPNESS):
        out += [(D.AugDesc(kind, factor=f), None) for f in factors]
    for deg in ((27.0, -30.0) if big else (30.0, -30.0, 27.0, -13.5)):
        out.append((D.AugDesc(D.AUG_AFFINE, fill=FILL, m=D._rotate_matrix(deg, w, h)), deg))
    for s in ((0.27, -0.3) if big else (0.3, -0.27)):
        out.append((D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, s, 0, 0, 1, 0)), None))
        out.append((D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, 0, 0, s, 1, 0)), None))
    for p in ((0.405, -0.45) if big else (0.45, -0.405)):
        out.append((D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, 0, p * w, 0, 1, 0)), None))
        out.append((D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, 0, 0, 0, 1, p * h)), None))
    return out


def flat(op):
    kind, arg, factor, fill, m = op
    return np.array([kind, arg, factor] + list(fill) + list(m), dtype=np.float64)


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    j = 0
    for i, img in enumerate(images()):
        out[f"img{i}"] = img
        h, w = img.shape[:2]
        for op, deg in cases(h, w, h * w > 10000):
            out[f"op{j}"] = np.concatenate([[i], flat(op)])
            out[f"out{j}"] = np.asarray(pillow(img, op, deg))
            j += 1
    path = os.path.join(HERE, "randaugment.npz")
    np.savez_compressed(path, **out)
    print("wrote", j, "cases,", os.path.getsize(path), "bytes; Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
