"""csrc/pruned_ops.hip on the device: the compact gradient finalisation bit for bit against cream_grad_finalize into a padded
buffer (and against the NumPy tree of tests/pruned_ref.py), pad / unpad bit for bit against F.pad / slicing plus cast."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pruned_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 8), (3, 5, 8), (1, 101, 104), (67, 101, 104), (128, 509, 512), (101, 128, 128)]      # (rows, cols, ld_src)
NPARTS = [1, 2, 5, 16, 17, 64, 65, 70]            # the part-lane classes 4 / 16 / 64 and their edges
GUARD = 8
SENTINEL = -123.0                 # (exact in bf16 too)


def _cases():
    """Every shape x nparts x partial dtype; overwrite and the destination offset cycle so that every shape meets all eight
    combinations of (dtype, overwrite, offset)."""
    out = []
    for si, shape in enumerate(SHAPES):
        for ni, nparts in enumerate(NPARTS):
            for bf in (0, 1):
                out.append(dict(shape=shape, nparts=nparts, bf16=bf, overwrite=(ni + bf) % 2, offset=(ni // 2 + bf + si) % 2))
    return out


def _make(case, gen):
    rows, cols, ld = case["shape"]
    n = case["nparts"]
    dt = torch.bfloat16 if case["bf16"] else torch.float32
    src = torch.randn((n, rows, ld), generator=gen, device=DEV, dtype=torch.float32).to(dt)
    src[:, :, cols:] = float("nan")                                     # a read of the padding into a result shows
    prefill = torch.randn((rows, ld), generator=gen, device=DEV, dtype=torch.float32)
    flat = torch.full((1 + rows * cols + GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
    off = case["offset"]                                                # 1: one float off the 16-byte alignment
    dst = flat[off:off + rows * cols].view(rows, cols)
    dst.copy_(prefill[:, :cols])
    return dict(case, src=src, padded=prefill.clone(), prefill=prefill, flat=flat, dst=dst)


def test_compact_finalize_equals_padded_finalize_and_slice():
    from cream_amd import _lib
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(5)
    items = [_make(c, gen) for c in _cases()]
    for shape in SHAPES:
        assert len({(i["bf16"], i["overwrite"], i["offset"]) for i in items if i["shape"] == shape}) == 8
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    per = 12                                                            # multi-job launches mixing shapes, dtypes and modes
    for s in range(0, len(items), per):
        group = items[s:s + per]
        ref = (_lib.GradJob * len(group))()
        new = (_lib.GradCompactJob * len(group))()
        for k, it in enumerate(group):
            rows, cols, ld = it["shape"]
            ref[k].dst, ref[k].src, ref[k].ld, ref[k].pstride = it["padded"].data_ptr(), it["src"].data_ptr(), ld, rows * ld
            ref[k].nparts, ref[k].rows, ref[k].cols, ref[k].src_bf16, ref[k].overwrite = it["nparts"], rows, ld, it["bf16"], it["overwrite"]
            new[k].dst, new[k].src, new[k].ld_dst, new[k].ld_src, new[k].pstride = it["dst"].data_ptr(), it["src"].data_ptr(), cols, ld, rows * ld
            new[k].nparts, new[k].rows, new[k].cols, new[k].src_bf16, new[k].overwrite = it["nparts"], rows, cols, it["bf16"], it["overwrite"]
            assert it["dst"].data_ptr() % 16 == 4 * it["offset"]
        _lib.check(lib.cream_grad_finalize(ctypes.cast(ref, ctypes.c_void_p), len(group), stream), "cream_grad_finalize")
        _lib.check(lib.cream_grad_finalize_compact(ctypes.cast(new, ctypes.c_void_p), len(group), stream), "cream_grad_finalize_compact")
    torch.cuda.synchronize()
    for it in items:
        rows, cols, ld = it["shape"]
        tag = {k: it[k] for k in ("shape", "nparts", "bf16", "overwrite", "offset")}
        assert not bool(torch.isnan(it["dst"]).any()), tag
        assert torch.equal(it["dst"], it["padded"][:, :cols]), tag
        off = it["offset"]
        assert bool((it["flat"][:off] == SENTINEL).all()) and bool((it["flat"][off + rows * cols:] == SENTINEL).all()), tag
        want = R.finalize_compact(it["prefill"][:, :cols].cpu().numpy(), it["src"].float().cpu().numpy(), rows, cols, ld, it["overwrite"])
        assert np.array_equal(it["dst"].cpu().numpy(), want), tag


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pad_and_unpad_are_exact(dtype):
    from cream_amd import _lib
    from cream_amd.tinyclip import pruned_ops as P
    gen = torch.Generator(device=DEV).manual_seed(9)
    for M in (1, 3, 259):
        for d in (1, 9, 101, 104):
            Dp = P.padded(d)
            assert Dp % 8 == 0 and 0 <= Dp - d < 8
            for off in (0, 1):                                          # the compact side one element off its natural 16 bytes
                flat = torch.randn(M * d + 1, generator=gen, device=DEV, dtype=torch.float32).to(dtype)
                x = flat[off:off + M * d].view(M, d)
                out = torch.full((M, Dp), float("nan"), device=DEV, dtype=torch.float32)
                assert P.pad_cols(x, Dp, out=out) is out
                want = F.pad(x.float(), (0, Dp - d))
                assert torch.equal(out, want) and bool((out[:, d:] == 0).all()), (M, d, off)
                assert np.array_equal(out.cpu().numpy(), R.pad_cols(x.float().cpu().numpy(), Dp))
            y = torch.randn((M, Dp), generator=gen, device=DEV, dtype=torch.float32)
            got = P.unpad_cols(y, d, dtype)
            assert got.shape == (M, d) and got.dtype == dtype and torch.equal(got, y[:, :d].to(dtype)), (M, d)
            # straight through the C ABI into a guarded, misaligned compact buffer: nothing beyond M x d is written
            flat = torch.full((M * d + 1 + GUARD,), SENTINEL, device=DEV, dtype=dtype)
            rc = _lib.load().cream_unpad_cols(ctypes.c_void_p(flat[1:].data_ptr()), _lib.BF16 if dtype == torch.bfloat16 else _lib.F32,
                                              ctypes.c_void_p(y.data_ptr()), M, d, Dp, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            assert torch.equal(flat[1:1 + M * d].view(M, d), got) and bool((flat[1 + M * d:] == SENTINEL).all()) and float(flat[0]) == SENTINEL
