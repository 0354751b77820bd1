"""GPU: RandAugment on the device (csrc/image_augment.hip through cream_image_augment_u8 / cream_image_batch_transform_aug, and
autoformer.data.DeviceTransform / DeviceBatches) against the numpy restatement of the 15 ops (tests/randaugment_ref.py, pinned
against Pillow on the CPU), the Pillow-made fixtures (tests/golden/randaugment.npz) and Pillow itself where it imports: BYTE-EXACT
uint8 images, BIT-EXACT fp32 batches."""
import ctypes
import random

import numpy as np
import pytest
import torch

import randaugment_ref as R
from oracle import image_transform_oracle as O
from cream_amd import _lib
from cream_amd.autoformer import data as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(__file__.rsplit("/", 1)[0] + "/golden/randaugment.npz")
FILL = (124, 116, 104)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def augment_u8(images, ops_per_image):
    """(B, H, W, 3) uint8 numpy + per image a list of AugDesc -> the device's (B, H, W, 3) uint8."""
    lib = _lib.load()
    B, H, W = images.shape[:3]
    arr, n = D.aug_op_array(ops_per_image)
    src = torch.from_numpy(np.ascontiguousarray(images)).to(DEV)
    dst = torch.empty_like(src)
    od = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    ws_bytes = lib.cream_image_augment_workspace(B, H, W, n)
    assert ws_bytes >= 0
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    rc = lib.cream_image_augment_u8(_p(dst), _p(src), B, H, W, arr, _p(od), n, _p(ws), ws_bytes, None)
    assert rc == 0
    return dst.cpu().numpy()


def every_op(h, w):
    """Every op kind at extreme and typical arguments (rotations / shears / translations at both signs)."""
    ops = [D.AugDesc(D.AUG_NONE), D.AugDesc(D.AUG_AUTOCONTRAST), D.AugDesc(D.AUG_EQUALIZE), D.AugDesc(D.AUG_INVERT)]
    ops += [D.AugDesc(D.AUG_POSTERIZE, arg=b) for b in (0, 1, 4, 8)]
    ops += [D.AugDesc(D.AUG_SOLARIZE, arg=t) for t in (0, 26, 128, 256)]
    ops += [D.AugDesc(D.AUG_SOLARIZE_ADD, arg=a) for a in (0, 99, 110)]
    for kind in (D.AUG_COLOR, D.AUG_CONTRAST, D.AUG_BRIGHTNESS, D.AUG_SHARPNESS):
        ops += [D.AugDesc(kind, factor=f) for f in (0.1, 0.19, 1.0, 1.81, 1.9)]
    ops += [D.AugDesc(D.AUG_AFFINE, fill=FILL, m=D._rotate_matrix(d, w, h)) for d in (30.0, -30.0, 27.0, -4.5)]
    for s in (0.3, -0.27):
        ops += [D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, s, 0, 0, 1, 0)), D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, 0, 0, s, 1, 0))]
    for p in (0.45, -0.405):
        ops += [D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, 0, p * w, 0, 1, 0)),
                D.AugDesc(D.AUG_AFFINE, fill=FILL, m=(1, 0, 0, 0, 1, p * h))]
    return ops


def _gold_cases():
    by_img = {}
    for k in GOLD.files:
        if k.startswith("op"):
            j = int(k[2:])
            v = GOLD[k]
            op = D.AugDesc(int(v[1]), int(v[2]), float(v[3]), tuple(int(x) for x in v[4:7]), tuple(float(x) for x in v[7:13]))
            by_img.setdefault(int(v[0]), []).append((op, GOLD[f"out{j}"]))
    return by_img


def test_fixtures_byte_exact_through_augment_u8():
    """Every Pillow-made case (1 x 1, 2 x 3, odd sizes, 224 x 224), one batch per image: the device's bytes are Pillow's and the
    restatement's."""
    for i, cases in sorted(_gold_cases().items()):
        img = GOLD[f"img{i}"]
        got = augment_u8(np.stack([img] * len(cases)), [[op] for op, _ in cases])
        for g, (op, want) in zip(got, cases):
            assert np.array_equal(g, want), (img.shape, op)
            assert np.array_equal(g, R.apply(img, op)), (img.shape, op)


@pytest.mark.parametrize("size", [224, 384])
def test_every_op_kind_byte_exact_at_training_sizes(size):
    """Random images at 224^2 and 384^2 (DeiT-384), every op kind in one batch, one op per image and then two per image."""
    rng = np.random.default_rng(size)
    ops = every_op(size, size)
    imgs = rng.integers(0, 256, (len(ops), size, size, 3), dtype=np.uint8)
    imgs[1] = np.clip(imgs[1], 60, 190)                      # autocontrast with a narrow histogram
    got = augment_u8(imgs, [[op] for op in ops])
    for g, img, op in zip(got, imgs, ops):
        assert np.array_equal(g, R.apply(img, op)), op
    chained = [[ops[i], ops[(i * 7 + 3) % len(ops)]] for i in range(len(ops))]
    got = augment_u8(imgs, chained)
    for g, img, chain in zip(got, imgs, chained):
        assert np.array_equal(g, R.apply_chain(img, chain)), chain


def _random_op(rng, h, w):
    kind = int(rng.integers(0, 12))
    if kind == D.AUG_POSTERIZE:
        return D.AugDesc(kind, arg=int(rng.integers(0, 9)))
    if kind == D.AUG_SOLARIZE:
        return D.AugDesc(kind, arg=int(rng.integers(0, 257)))
    if kind == D.AUG_SOLARIZE_ADD:
        return D.AugDesc(kind, arg=int(rng.integers(0, 111)))
    if kind in (D.AUG_COLOR, D.AUG_CONTRAST, D.AUG_BRIGHTNESS, D.AUG_SHARPNESS):
        return D.AugDesc(kind, factor=float(rng.uniform(0.0, 2.2)))
    if kind == D.AUG_AFFINE:
        if rng.random() < 0.5:
            return D.AugDesc(kind, fill=FILL, m=D._rotate_matrix(float(rng.uniform(-30, 30)), w, h))
        m = tuple(rng.uniform(-1.3, 1.3, 6) * np.array([1, 1, w, 1, 1, h]))            # taps on every edge, all directions
        return D.AugDesc(kind, fill=tuple(int(v) for v in rng.integers(0, 256, 3)), m=m)
    return D.AugDesc(kind)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_fuzz_batch_128_random_ops_per_image(n):
    rng = np.random.default_rng(100 + n)
    h, w = 37, 52
    imgs = rng.integers(0, 256, (128, h, w, 3), dtype=np.uint8)
    chains = [[_random_op(rng, h, w) for _ in range(n)] for _ in range(128)]
    got = augment_u8(imgs, chains)
    for b in range(128):
        assert np.array_equal(got[b], R.apply_chain(imgs[b], chains[b])), (b, chains[b])


SHAPES = [(375, 500), (500, 375), (333, 500), (224, 224), (64, 80), (768, 1024), (1200, 900), (100, 400)]


def test_imagenet_shaped_batch_with_rand_augment_bit_exact():
    """Ragged ImageNet-shaped frames, training crops + mirrors, RandAugment draws of the recipe's policy (+ an extra chain of every
    whole-image op), RandomErasing boxes: the fp32 batch is bit for bit crop / resize / mirror (the oracle) -> the restatement's ops
    -> ToTensor / Normalize outside the boxes, the device's noise inside them."""
    rng = np.random.default_rng(11)
    pr, nr = random.Random(5), np.random.RandomState(3)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    policy = D.parse_rand_augment('rand-m9-mstd0.5-inc1')
    params, chains = [], []
    for i, (h, w) in enumerate(SHAPES):
        box, resized, window, flip = D.train_crop_params(h, w, pr)
        ops = D.rand_augment_params(pr, nr, policy, 224, 224)
        ops[i % 2] = [D.AugDesc(D.AUG_EQUALIZE), D.AugDesc(D.AUG_AUTOCONTRAST), D.AugDesc(D.AUG_CONTRAST, factor=0.37),
                      D.AugDesc(D.AUG_SHARPNESS, factor=1.63)][i % 4]
        erase = D.random_erasing_params(pr, 224, 224, 0.6)
        params.append((box, resized, window, flip, erase))
        chains.append(ops)
    out = D.DeviceTransform(224, device=DEV)(frames, params, aug_ops=chains).cpu()
    erased = 0
    for o, f, (box, resized, window, flip, erase), ops in zip(out, frames, params, chains):
        u8 = R.apply_chain(np.ascontiguousarray(O.resized_window(f, box, resized, window, (224, 224), flip)), ops)
        want = O.to_tensor_normalize(u8)
        keep = torch.ones(224, 224, dtype=torch.bool)
        if erase is not None:
            t, l, h, w, seed = erase
            keep[t:t + h, l:l + w] = False
            noise = torch.from_numpy(D.erase_noise_reference(seed, 3, 224, 224))
            assert float((o[:, ~keep] - noise[:, ~keep]).abs().max()) < 1e-4
            erased += 1
        assert torch.equal(o[:, keep], want[:, keep])
    assert erased >= 1


def test_all_none_ops_equal_the_plain_transform():
    rng = np.random.default_rng(12)
    pr = random.Random(8)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    params = [D.train_crop_params(h, w, pr) + (D.random_erasing_params(pr, 224, 224, 0.5),) for h, w in SHAPES]
    T = D.DeviceTransform(224, device=DEV)
    plain = T(frames, params)
    for n in (1, 2, 3):
        aug = T(frames, params, aug_ops=[[D.AugDesc(D.AUG_NONE)] * n for _ in frames])
        assert torch.equal(aug, plain), n
    T384 = D.DeviceTransform(384, device=DEV)
    p384 = [D.train_crop_params(h, w, pr, 384) for h, w in SHAPES[:3]]
    assert torch.equal(T384(frames[:3], p384, aug_ops=[[D.AugDesc(D.AUG_NONE)] * 2] * 3), T384(frames[:3], p384))


def test_c_abi_rejects_bad_ops_before_any_launch():
    lib = _lib.load()
    T = D.DeviceTransform(224, device=DEV)
    arr, n = D.aug_op_array([[D.AugDesc(D.AUG_INVERT)]])
    descs, nbytes, ws = T.plan([(300, 400)], [D.eval_crop_params(300, 400)], (arr, n))
    pix = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    od = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    out = torch.empty(1, 3, 224, 224, device=DEV)
    wsb = torch.empty(ws, dtype=torch.uint8, device=DEV)
    call = lambda a, w: lib.cream_image_batch_transform_aug(_p(out), _p(pix), nbytes, descs, _p(dd), 1, 224, 224, T._mean, T._std, a,
                                                            _p(od), 1, _p(wsb), w, None)
    assert call(arr, ws) == 0
    assert call(arr, ws - 16) == -1
    arr[0].kind = 12
    assert call(arr, ws) == -1
    torch.cuda.synchronize()


def test_device_batches_with_rand_augment_match_the_same_draws_on_the_host():
    """DeviceBatches(mode='train', auto_augment='rand-m9-mstd0.5-inc1'): crop / flip, RandAugment and RandomErasing drawn per image
    in timm's order; the same draws replayed give the same tensors (the host pipeline outside the erased boxes), and the ops drawn
    are the host restatement's."""
    rng = np.random.default_rng(6)
    shapes = [(300, 400), (260, 260), (500, 333), (240, 320)] * 4
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    loader = [(frames, list(range(16)))]
    T = D.DeviceTransform(224, device=DEV)
    mk = lambda: D.DeviceBatches(loader, T, "train", rng=random.Random(11), reprob=0.25, auto_augment='rand-m9-mstd0.5-inc1',
                                 np_rng=np.random.RandomState(4))
    (x, y), = list(mk())
    assert y.tolist() == list(range(16)) and tuple(x.shape) == (16, 3, 224, 224)
    replay = mk().params_for(shapes)
    applied = 0
    for o, f, (box, resized, window, flip, erase, ops) in zip(x.cpu(), frames, replay):
        assert len(ops) == 2
        applied += sum(op.kind != D.AUG_NONE for op in ops)
        want = O.to_tensor_normalize(R.apply_chain(np.ascontiguousarray(O.resized_window(f, box, resized, window, (224, 224), flip)),
                                                   ops))
        keep = torch.ones(224, 224, dtype=torch.bool)
        if erase is not None:
            t, l, h, w, _ = erase
            keep[t:t + h, l:l + w] = False
        assert torch.equal(o[:, keep], want[:, keep])
    assert 4 <= applied <= 28
    try:
        from PIL import Image, ImageOps
    except ImportError:
        return
    # one literal Pillow check: an Invert-only chain is ImageOps.invert of Pillow's crop / resize / mirror
    f = frames[0]
    prm = ((0, 0, 300, 400), (224, 224), (0, 0), True)
    got = T([f], [prm], aug_ops=[[D.AugDesc(D.AUG_INVERT), D.AugDesc(D.AUG_NONE)]]).cpu()[0]
    im = Image.fromarray(f).resize((224, 224), Image.BICUBIC).transpose(Image.FLIP_LEFT_RIGHT)
    assert torch.equal(got, O.to_tensor_normalize(np.asarray(ImageOps.invert(im))))
