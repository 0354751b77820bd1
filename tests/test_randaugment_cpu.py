"""CPU: RandAugment of the training recipe — the numpy restatement of the 15 ops (tests/randaugment_ref.py) against the installed
Pillow and the Pillow-made fixtures, the host descriptors (autoformer.data.rand_augment_params) against timm's literal Pillow calls,
the policy grammar, the draws, and the C ABI's host-side planning / validation (no device needed)."""
import ctypes
import random

import numpy as np
import pytest

import randaugment_ref as R
from cream_amd import _lib
from cream_amd.autoformer import data as D

Image = pytest.importorskip("PIL.Image")
from PIL import ImageEnhance, ImageOps  # noqa: E402

GOLD = np.load(__file__.rsplit("/", 1)[0] + "/golden/randaugment.npz")
FILL = (124, 116, 104)


def _images(seed):
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((1, 1), (2, 3), (3, 2), (5, 7), (40, 52), (31, 17))]
    out.append(rng.integers(90, 140, (12, 9, 3), dtype=np.uint8))
    out.append(rng.choice(np.array([3, 250], dtype=np.uint8), (6, 10, 3)))
    eq = np.zeros((1, 512, 3), dtype=np.uint8)                      # equalize's LUT reaches 256 at the last bin: clipped to 255
    eq[0, -1] = 255
    out.append(eq)
    return out


def test_lut_and_blend_ops_equal_pillow():
    for img in _images(1):
        im = Image.fromarray(img)
        assert np.array_equal(R.apply(img, D.AugDesc(D.AUG_AUTOCONTRAST)), np.asarray(ImageOps.autocontrast(im)))
        assert np.array_equal(R.apply(img, D.AugDesc(D.AUG_EQUALIZE)), np.asarray(ImageOps.equalize(im)))
        assert np.array_equal(R.apply(img, D.AugDesc(D.AUG_INVERT)), np.asarray(ImageOps.invert(im)))
        for b in range(9):
            assert np.array_equal(R.apply(img, D.AugDesc(D.AUG_POSTERIZE, arg=b)), np.asarray(ImageOps.posterize(im, b)))
        for t in (0, 1, 26, 128, 255, 256):
            assert np.array_equal(R.apply(img, D.AugDesc(D.AUG_SOLARIZE, arg=t)), np.asarray(ImageOps.solarize(im, t)))
        for a in (0, 50, 110):
            want = im.point([min(255, i + a) if i < 128 else i for i in range(256)] * 3)
            assert np.array_equal(R.apply(img, D.AugDesc(D.AUG_SOLARIZE_ADD, arg=a)), np.asarray(want))
        for f in (0.0, 0.1, 0.37, 1.0, 1.63, 1.9, 1.0 + 0.9 * 0.87, 2.4):
            for kind, cls in ((D.AUG_COLOR, ImageEnhance.Color), (D.AUG_CONTRAST, ImageEnhance.Contrast),
                              (D.AUG_BRIGHTNESS, ImageEnhance.Brightness), (D.AUG_SHARPNESS, ImageEnhance.Sharpness)):
                assert np.array_equal(R.apply(img, D.AugDesc(kind, factor=f)), np.asarray(cls(im).enhance(f))), (kind, f, img.shape)


def test_affine_fuzz_equals_pillow_on_every_edge():
    """Random matrices that put taps beyond every edge in all four directions, shears, translations and rotations of +-30 degrees
    (Image.rotate's own call, against the generic affine op with the host's matrix)."""
    rng = np.random.default_rng(2)
    for img in _images(3)[:8]:
        h, w = img.shape[:2]
        im = Image.fromarray(img)
        for _ in range(12):
            m = tuple(rng.uniform(-1.4, 1.4, 6) * np.array([1, 1, w, 1, 1, h]))
            fill = tuple(int(v) for v in rng.integers(0, 256, 3))
            want = im.transform(im.size, Image.AFFINE, m, Image.BICUBIC, fillcolor=fill)
            assert np.array_equal(R.apply(img, D.AugDesc(D.AUG_AFFINE, fill=fill, m=m)), np.asarray(want)), (img.shape, m)
        for deg in (30.0, -30.0, 29.7, -0.3, 12.0, 0.0):
            want = im.rotate(deg, resample=Image.BICUBIC, fillcolor=FILL)
            got = R.apply(img, D.AugDesc(D.AUG_AFFINE, fill=FILL, m=D._rotate_matrix(deg, w, h)))
            assert np.array_equal(got, np.asarray(want)), (img.shape, deg)


def test_restatement_equals_the_fixtures():
    n = 0
    for k in GOLD.files:
        if k.startswith("op"):
            v = GOLD[k]
            op = D.AugDesc(int(v[1]), int(v[2]), float(v[3]), tuple(int(x) for x in v[4:7]), tuple(float(x) for x in v[7:13]))
            assert np.array_equal(R.apply(GOLD[f"img{int(v[0])}"], op), GOLD[f"out{k[2:]}"]), op
            n += 1
    kinds = {int(GOLD[k][1]) for k in GOLD.files if k.startswith("op")}
    assert n > 200 and kinds == set(range(12))


def _timm_call(im, name, level, fill, rnd):
    """timm 0.3.2's aug_fn(img, *level_fn(level)) with its sign draw from `rnd` — the literal Pillow calls of auto_augment.py."""
    neg = lambda v: -v if rnd.random() > 0.5 else v                                              # noqa: E731
    if name == 'AutoContrast':
        return ImageOps.autocontrast(im)
    if name == 'Equalize':
        return ImageOps.equalize(im)
    if name == 'Invert':
        return ImageOps.invert(im)
    if name == 'Rotate':
        return im.rotate(neg((level / 10.) * 30.), resample=Image.BICUBIC, fillcolor=fill)
    if name == 'PosterizeIncreasing':
        bits = 4 - int((level / 10.) * 4)
        return im if bits >= 8 else ImageOps.posterize(im, bits)
    if name == 'SolarizeIncreasing':
        return ImageOps.solarize(im, 256 - int((level / 10.) * 256))
    if name == 'SolarizeAdd':
        add = int((level / 10.) * 110)
        return im.point([min(255, i + add) if i < 128 else i for i in range(256)] * 3)
    if name.endswith('Increasing'):
        cls = getattr(ImageEnhance, name[:-len('Increasing')])
        return cls(im).enhance(1.0 + neg((level / 10.) * .9))
    if name == 'ShearX':
        return im.transform(im.size, Image.AFFINE, (1, neg((level / 10.) * 0.3), 0, 0, 1, 0), resample=Image.BICUBIC, fillcolor=fill)
    if name == 'ShearY':
        return im.transform(im.size, Image.AFFINE, (1, 0, 0, neg((level / 10.) * 0.3), 1, 0), resample=Image.BICUBIC, fillcolor=fill)
    pct = neg((level / 10.) * 0.45)
    if name == 'TranslateXRel':
        return im.transform(im.size, Image.AFFINE, (1, 0, pct * im.size[0], 0, 1, 0), resample=Image.BICUBIC, fillcolor=fill)
    return im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, pct * im.size[1]), resample=Image.BICUBIC, fillcolor=fill)


def _timm_rand_augment(img, rnd, np_rnd, M=9, N=2, S=0.5, fill=FILL):
    """RandAugment.__call__ / AugmentOp.__call__ of timm 0.3.2 with prob 0.5, on a PIL image, drawing from (rnd, np_rnd)."""
    im = Image.fromarray(img)
    for idx in np_rnd.choice(15, N):
        if rnd.random() > 0.5:
            continue
        m = rnd.gauss(M, S) if S > 0 else M
        m = min(10., max(0, m))
        im = _timm_call(im, D.RAND_INCREASING_TRANSFORMS[int(idx)], m, fill, rnd)
    return np.asarray(im)


@pytest.mark.parametrize("hw", [(224, 224), (37, 53), (384, 384)])
def test_host_descriptors_equal_the_literal_timm_pillow_calls(hw):
    """The descriptors of rand_augment_params applied by the restatement == timm's op calls on Pillow with the same draws."""
    h, w = hw
    rng = np.random.default_rng(h * w)
    reps = 40 if h * w < 100000 else 10
    for seed in range(reps):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ops = D.rand_augment_params(random.Random(seed), np.random.RandomState(seed), 'rand-m9-mstd0.5-inc1', h, w)
        want = _timm_rand_augment(img, random.Random(seed), np.random.RandomState(seed))
        assert np.array_equal(R.apply_chain(img, ops), want), (seed, ops)
    # every op name at both signs of the recipe's magnitude, without the gate
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for name in D.RAND_INCREASING_TRANSFORMS:
        for seed in range(4):
            want = np.asarray(_timm_call(Image.fromarray(img), name, 9, FILL, random.Random(seed)))
            got = R.apply(img, _single_desc(name, 9, random.Random(seed), h, w))
            assert np.array_equal(got, want), (name, seed)


def _single_desc(name, level, rnd, h, w):
    """rand_augment_params for one op that passed its gate: replays the gate draw as 'apply' and magnitude `level`."""
    class Gate:
        def __init__(self):
            self.first = True

        def random(self):
            if self.first:
                self.first = False
                return 0.0
            return rnd.random()

        def gauss(self, mu, sigma):
            return mu

    class Choice:
        def choice(self, n, size):
            return [D.RAND_INCREASING_TRANSFORMS.index(name)]

    return D.rand_augment_params(Gate(), Choice(), D.RandAugmentPolicy((level, 1, 0.0, FILL)), h, w)[0]


def test_policy_parsing():
    p = D.parse_rand_augment('rand-m9-mstd0.5-inc1')
    assert (p.magnitude, p.num_layers, p.magnitude_std, p.fill) == (9, 2, 0.5, (124, 116, 104))
    assert D.parse_rand_augment('rand-inc1-m7-n3') == (7, 3, 0.0, (124, 116, 104))
    assert D.parse_rand_augment('rand-m9-inc1', mean=(0.48145466, 0.4578275, 0.40821073)).fill == (123, 117, 104)
    for bad in ('rand-m9-mstd0.5', 'rand-m9-mstd0.5-inc0', 'rand-m9-inc1-w0', 'rand-n2-inc1', 'rand-m9-inc1-x3', 'augmix-m5',
                'original-mstd0.5', 'rand-m9-inc1-mstd', None):
        with pytest.raises(ValueError):
            D.parse_rand_augment(bad)
    with pytest.raises(ValueError):
        D.parse_rand_augment('rand-m9-mstd0.5-inc1', interpolation='random')
    with pytest.raises(ValueError):
        D.parse_rand_augment('rand-m9-mstd0.5-inc1', interpolation='bilinear')
    with pytest.raises(ValueError):
        D.DeviceBatches([], D.DeviceTransform(224, device="cpu"), "eval", auto_augment='rand-m9-mstd0.5-inc1')
    with pytest.raises(ValueError):
        D.DeviceBatches([], D.DeviceTransform(224, device="cpu"), "train", auto_augment='rand-m9-inc0')


def test_draw_properties():
    """The gate skips about half the ops, magnitudes stay in [0, 10] (mstd 5 clips at both ends), the op indices are
    np_rng.choice(15, N)'s, and the draw count per image is timm's."""
    rnd, nr = random.Random(1), np.random.RandomState(2)
    policy = D.parse_rand_augment('rand-m9-mstd0.5-inc1')
    ops = [op for _ in range(2000) for op in D.rand_augment_params(rnd, nr, policy, 224, 224)]
    skipped = sum(op.kind == D.AUG_NONE for op in ops) / len(ops)
    assert 0.47 < skipped < 0.53
    assert {op.kind for op in ops} == set(range(12))
    for op in ops:
        if op.kind == D.AUG_POSTERIZE:
            assert 0 <= op.arg <= 4
        elif op.kind == D.AUG_SOLARIZE:
            assert 0 <= op.arg <= 256
        elif op.kind == D.AUG_SOLARIZE_ADD:
            assert 0 <= op.arg <= 110
        elif op.kind in (D.AUG_COLOR, D.AUG_CONTRAST, D.AUG_BRIGHTNESS, D.AUG_SHARPNESS):
            assert 0.1 - 1e-12 <= op.factor <= 1.9 + 1e-12
    wide = [op for _ in range(1000) for op in D.rand_augment_params(rnd, nr, 'rand-m5-mstd5-inc1', 224, 224)]
    f = [abs(op.factor - 1.0) for op in wide if op.kind in (D.AUG_COLOR, D.AUG_CONTRAST, D.AUG_BRIGHTNESS, D.AUG_SHARPNESS)]
    assert max(f) == pytest.approx(0.9) and min(f) == 0.0                      # clipped at 10 and at 0
    # op indices: numpy's choice, consumed once per image before the python draws
    nr1, nr2 = np.random.RandomState(7), np.random.RandomState(7)
    for _ in range(50):
        idx = nr2.choice(15, 2)
        ops = D.rand_augment_params(random.Random(0), nr1, D.RandAugmentPolicy((9, 2, 0.0, FILL)), 224, 224)
        r = random.Random(0)
        for i, op in zip(idx, ops):
            gate = r.random() > 0.5
            name = D.RAND_INCREASING_TRANSFORMS[int(i)]
            assert (op.kind == D.AUG_NONE) == gate
            if not gate and name in ('Rotate', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel', 'ColorIncreasing',
                                     'ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing'):
                r.random()
    # with auto_augment=None DeviceBatches draws exactly what it drew before
    b0 = D.DeviceBatches([], D.DeviceTransform(224, device="cpu"), "train", rng=random.Random(3), reprob=0.25)
    rr = random.Random(3)
    want = []
    for h, w in [(300, 400), (500, 333)]:
        want.append(D.train_crop_params(h, w, rr, 224) + (D.random_erasing_params(rr, 224, 224, 0.25),))
    assert b0.params_for([(300, 400), (500, 333)]) == want
    b1 = D.DeviceBatches([], D.DeviceTransform(224, device="cpu"), "train", rng=random.Random(3), reprob=0.25,
                         auto_augment='rand-m9-mstd0.5-inc1', np_rng=np.random.RandomState(5))
    rr, nr = random.Random(3), np.random.RandomState(5)
    want = []
    for h, w in [(300, 400), (500, 333)]:
        crop = D.train_crop_params(h, w, rr, 224)
        ops = D.rand_augment_params(rr, nr, 'rand-m9-mstd0.5-inc1', 224, 224)
        want.append(crop + (D.random_erasing_params(rr, 224, 224, 0.25), ops))
    assert b1.params_for([(300, 400), (500, 333)]) == want


def test_plan_aug_sizes_the_workspace_and_rejects_bad_descriptors():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.AugOp) == 64
    T = D.DeviceTransform(224, device="cpu")
    shapes, params = [(300, 400), (500, 375)], [D.eval_crop_params(300, 400), D.eval_crop_params(500, 375)]
    descs, _, plain = T.plan(shapes, params)
    for n, bufs in ((1, 1), (2, 2), (4, 2)):
        arr, n_ = D.aug_op_array([[D.AugDesc(D.AUG_INVERT)] * n] * 2)
        ws = lib.cream_image_batch_plan_aug(descs, 2, 224, 224, arr, n_)
        assert ws >= plain + bufs * 2 * 224 * 224 * 4 and ws % 16 == 0, (n, ws, plain)
    assert lib.cream_image_batch_plan_aug(descs, 2, 224, 224, arr, 0) == plain
    bad = [D.AugDesc(12), D.AugDesc(-1), D.AugDesc(D.AUG_POSTERIZE, arg=9), D.AugDesc(D.AUG_POSTERIZE, arg=-1),
           D.AugDesc(D.AUG_SOLARIZE, arg=257), D.AugDesc(D.AUG_SOLARIZE_ADD, arg=256), D.AugDesc(D.AUG_COLOR, factor=float("nan")),
           D.AugDesc(D.AUG_SHARPNESS, factor=float("inf")), D.AugDesc(D.AUG_AFFINE, m=(1, 0, float("nan"), 0, 1, 0)),
           D.AugDesc(D.AUG_AFFINE, m=(1, 0, 0, 0, float("-inf"), 0))]
    for op in bad:
        arr, n = D.aug_op_array([[D.AugDesc(D.AUG_NONE), op], [D.AugDesc(D.AUG_NONE)] * 2])
        assert lib.cream_image_batch_plan_aug(descs, 2, 224, 224, arr, n) == -1, op
        assert lib.cream_image_augment_u8(None, None, 2, 8, 8, arr, None, n, None, 0, None) == -1
    arr, n = D.aug_op_array([[D.AugDesc(D.AUG_POSTERIZE, arg=8), D.AugDesc(D.AUG_SOLARIZE, arg=256)]] * 2)
    assert lib.cream_image_batch_plan_aug(descs, 2, 224, 224, arr, n) > 0
    assert lib.cream_image_batch_plan_aug(descs, 2, 224, 224, arr, 17) == -1                # > CREAM_AUG_MAX_OPS
    assert lib.cream_image_augment_workspace(128, 224, 224, 1) == 0
    assert lib.cream_image_augment_workspace(128, 224, 224, 2) == 128 * 224 * 224 * 4
    assert lib.cream_image_augment_workspace(128, 224, 224, 3) == 2 * 128 * 224 * 224 * 4
    assert lib.cream_image_augment_workspace(1, 8, 1025, 2) == -1
