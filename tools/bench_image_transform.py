"""The device input transform (cream_image_batch_transform) on a batch of 128 ImageNet-shaped frames: kernel time of the two launches
(HIP events on the launch stream, frames already resident in HBM), the end-to-end call with the host packing and the PCIe copy, and
Pillow + torch on the host cores beside it (the reference's per-image path, one thread).
    python tools/bench_image_transform.py [eval|train|train-aa]   ->  one JSON line
train-aa: the training transform with RandAugment ('rand-m9-mstd0.5-inc1', cream_image_batch_transform_aug): kernel time per batch
with and without the augmentation launches (the same crops, mirrors and erasing boxes), and Pillow's own RandAugment per image
on one core (timm's ops on the 224 x 224 crop)."""
import ctypes
import json
import random
import sys
import time

import numpy as np
import torch

import os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cream_amd import _lib                                   # noqa: E402
from cream_amd.autoformer import data as D                   # noqa: E402


def _timed(call, st, reps=20):
    for _ in range(3):
        assert call() == 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(st)
    for _ in range(reps):
        call()
    ev[1].record(st)
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def pillow_rand_augment(im, ops):
    """timm's op calls for the AugDesc chain of one image (the host path the device replaces)."""
    from PIL import Image, ImageEnhance, ImageOps
    for kind, arg, factor, fill, m in ops:
        if kind == D.AUG_AUTOCONTRAST:
            im = ImageOps.autocontrast(im)
        elif kind == D.AUG_EQUALIZE:
            im = ImageOps.equalize(im)
        elif kind == D.AUG_INVERT:
            im = ImageOps.invert(im)
        elif kind == D.AUG_POSTERIZE:
            im = ImageOps.posterize(im, arg)
        elif kind == D.AUG_SOLARIZE:
            im = ImageOps.solarize(im, arg)
        elif kind == D.AUG_SOLARIZE_ADD:
            im = im.point([min(255, i + arg) if i < 128 else i for i in range(256)] * 3)
        elif kind in (D.AUG_COLOR, D.AUG_CONTRAST, D.AUG_BRIGHTNESS, D.AUG_SHARPNESS):
            im = {D.AUG_COLOR: ImageEnhance.Color, D.AUG_CONTRAST: ImageEnhance.Contrast, D.AUG_BRIGHTNESS: ImageEnhance.Brightness,
                  D.AUG_SHARPNESS: ImageEnhance.Sharpness}[kind](im).enhance(factor)
        elif kind == D.AUG_AFFINE:
            im = im.transform(im.size, Image.AFFINE, m, Image.BICUBIC, fillcolor=fill)
    return im


def main_train_aa():
    B, size, dev = 128, 224, "cuda:0"
    rng = np.random.default_rng(0)
    pr, nr = random.Random(0), np.random.RandomState(0)
    mix = [(375, 500), (500, 375), (333, 500)]                   # ImageNet's three most common frame sizes
    shapes = [mix[i % len(mix)] for i in range(B)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    policy = D.parse_rand_augment("rand-m9-mstd0.5-inc1")
    params, chains = [], []
    for h, w in shapes:                                          # timm's order of draws per image
        crop = D.train_crop_params(h, w, pr)
        chains.append(D.rand_augment_params(pr, nr, policy, size, size))
        params.append(crop + (D.random_erasing_params(pr, size, size, 0.25),))
    T = D.DeviceTransform(size, device=dev)
    arr, n = D.aug_op_array(chains)
    descs, nbytes, ws = T.plan(shapes, params, (arr, n))
    pix = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for d, f in zip(descs, frames):
        pix[d.offset:d.offset + f.size] = torch.from_numpy(f.reshape(-1)).to(dev)
    dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    od = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    wsb = torch.empty(ws, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, size, size, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = _lib.load()
    st = torch.cuda.current_stream()
    s = ctypes.c_void_p(st.cuda_stream)
    plain = lambda: lib.cream_image_batch_transform(p(out), p(pix), nbytes, descs, p(dd), B, size, size, T._mean, T._std, p(wsb), ws, s)
    aug = lambda: lib.cream_image_batch_transform_aug(p(out), p(pix), nbytes, descs, p(dd), B, size, size, T._mean, T._std, arr, p(od),
                                                      n, p(wsb), ws, s)
    ms_plain, ms_aug = [], []
    for _ in range(3):                                           # alternated, median of three windows each
        ms_plain.append(_timed(plain, st))
        ms_aug.append(_timed(aug, st))
    ms_plain, ms_aug = sorted(ms_plain)[1], sorted(ms_aug)[1]
    applied = sum(op.kind != D.AUG_NONE for c in chains for op in c)
    cpu = None
    try:
        from PIL import Image
        crops = [np.ascontiguousarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)) for _ in range(64)]
        t0 = time.perf_counter()
        for c, ops in zip(crops, chains):
            pillow_rand_augment(Image.fromarray(c), ops)
        cpu = (time.perf_counter() - t0) / len(crops)
    except ImportError:
        pass
    print(json.dumps({"workload": f"input transform (train, RandAugment rand-m9-mstd0.5-inc1, reprob 0.25): {B} decoded frames "
                                  f"(333x500 .. 500x375) -> ({B}, 3, {size}, {size}) fp32",
                      "kernels_ms_plain": round(ms_plain, 4), "kernels_ms_with_rand_augment": round(ms_aug, 4),
                      "rand_augment_us_per_128_frames": round((ms_aug - ms_plain) * 1e3, 1), "estimate_us_per_128_frames": 50,
                      "ops_per_image": n, "ops_applied_in_batch": applied,
                      "images_per_sec_kernels_with_rand_augment": round(B / ms_aug * 1e3),
                      "cpu_pillow_rand_augment_ms_per_image_1_core": None if cpu is None else round(cpu * 1e3, 3)}))


def main():
    pipeline = sys.argv[1] if len(sys.argv) > 1 else "train"
    if pipeline == "train-aa":
        return main_train_aa()
    B, size, dev = 128, 224, "cuda:0"
    rng = np.random.default_rng(0)
    pr = random.Random(0)
    # ImageNet's typical frames: 500 x 375 / 375 x 500 / 500 x 333, a few larger ones
    mix = [(375, 500), (500, 375), (333, 500), (480, 640), (768, 1024)]
    if len(sys.argv) > 2 and sys.argv[2] == "typical":            # ImageNet's three most common frame sizes only
        mix = mix[:3]
    shapes = [mix[i % len(mix)] for i in range(B)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    params = [D.eval_crop_params(h, w) + (False,) if pipeline == "eval" else D.train_crop_params(h, w, pr) for h, w in shapes]
    T = D.DeviceTransform(size, device=dev)
    out = T(frames, params)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        out = T(frames, params)
    torch.cuda.synchronize()
    e2e = (time.perf_counter() - t0) / 5
    # kernels only: frames and descriptors resident
    descs, nbytes, ws = T.plan(shapes, params)
    pix = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for d, f in zip(descs, frames):
        pix[d.offset:d.offset + f.size] = torch.from_numpy(f.reshape(-1)).to(dev)
    dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    wsb = torch.empty(ws, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = _lib.load()
    st = torch.cuda.current_stream()
    call = lambda: lib.cream_image_batch_transform(p(out), p(pix), nbytes, descs, p(dd), B, size, size, T._mean, T._std, p(wsb), ws,
                                                   ctypes.c_void_p(st.cuda_stream))
    for _ in range(3):
        assert call() == 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(st)
    for _ in range(20):
        call()
    ev[1].record(st)
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / 20
    box_bytes = sum(d.nrows * d.box_w * 3 for d in descs)
    algo = box_bytes + 2 * sum(d.nrows * size * 3 for d in descs) + B * 3 * size * size * 4
    # the host path on one core: Pillow's crop + resize + crop, then the two float ops
    from PIL import Image
    t0 = time.perf_counter()
    n = 32
    for f, (box, resized, window, flip) in list(zip(frames, params))[:n]:
        t, l, h, w = box
        im = Image.fromarray(f).crop((l, t, l + w, t + h)).resize((resized[1], resized[0]), Image.BICUBIC)
        im = im.crop((window[1], window[0], window[1] + size, window[0] + size))
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        x = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div(255)
        x = x.sub(torch.tensor(D.IMAGENET_DEFAULT_MEAN).view(3, 1, 1)).div(torch.tensor(D.IMAGENET_DEFAULT_STD).view(3, 1, 1))
    cpu = (time.perf_counter() - t0) / n
    print(json.dumps({"workload": f"input transform ({pipeline}): {B} decoded frames ({min(s[0] for s in shapes)}x{min(s[1] for s in shapes)} .. {max(s[0] for s in shapes)}x{max(s[1] for s in shapes)}) -> (128, 3, 224, 224) fp32",
                      "kernels_ms": round(ms, 4), "images_per_sec_kernels": round(B / ms * 1e3), "algorithmic_bytes": algo,
                      "GBps": round(algo / ms / 1e6, 1), "frac_of_8TBps": round(algo / ms / 1e6 / 8000, 3),
                      "end_to_end_ms_with_host_packing_and_pcie": round(e2e * 1e3, 3),
                      "images_per_sec_end_to_end": round(B / e2e), "packed_MB": round(nbytes / 1e6, 1),
                      "cpu_pillow_torch_ms_per_image_1_core": round(cpu * 1e3, 3), "cpu_images_per_sec_1_core": round(1 / cpu, 1)}))


if __name__ == "__main__":
    main()
