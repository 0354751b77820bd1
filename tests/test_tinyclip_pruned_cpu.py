"""Pruned TinyCLIP towers on the native node, the parts that need no device: the plan and the decision of
cream_amd/tinyclip/native_pruned.py on a toy tower pruned by hand-set 0 / 1 masks (tests/pruned_ref.py), the host check of the
compact gradient finalisation, and the NumPy restatement of its summation tree against an fp64 sum."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pruned_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def tower():
    return R.toy_tower(101)


def test_plan_of_the_toy_tower(tower):
    from cream_amd.tinyclip import native_pruned
    pl = native_pruned.plan(tower)
    assert tower.width == 128                                             # keeps its pre-prune value
    assert (pl["d"], pl["Dp"]) == (101, 104)
    assert [b["attn"] for b in pl["blocks"]] == [True, True, False, True, False]
    assert [b["mlp"] for b in pl["blocks"]] == [True, True, True, False, False]
    assert [b["H"] for b in pl["blocks"]] == [2, 1, 0, 2, 0]
    assert [b["F"] for b in pl["blocks"]] == [509, 64, 8, 0, 0]
    assert [b["Fp"] for b in pl["blocks"]] == [512, 64, 8, 0, 0]
    assert native_pruned.plan(tower, 101) == pl and native_pruned.plan(tower, 104) is None     # x.shape[-1] has to agree
    assert native_pruned.plan(R.toy_tower(96))["Dp"] == 96 and native_pruned.plan(R.toy_tower(9))["Dp"] == 16


def test_supported_takes_the_pruned_tower_and_native_refuses_it(tower, monkeypatch):
    from cream_amd.tinyclip import native, native_pruned
    monkeypatch.setattr(native, "_environment_ok", lambda *a, **k: True)
    x = torch.zeros(2, 5, 101)
    assert native_pruned.supported(tower, x, None) is True
    assert native_pruned.supported(tower, x, torch.zeros(5, 5), causal=True) is True
    assert native.supported(tower, x, None) is False
    assert native_pruned.supported(tower, x, torch.zeros(5, 5)) is False                      # any other mask: composed
    assert native_pruned.supported(tower, torch.zeros(2, 5, 128), None) is False
    assert native_pruned.supported(tower, torch.zeros(2, 3000, 101), None) is False


def test_supported_refusals(monkeypatch):
    from cream_amd.tinyclip import native, native_pruned
    from cream_amd.tinyclip.model import QuickGELU
    monkeypatch.setattr(native, "_environment_ok", lambda *a, **k: True)
    x = torch.zeros(2, 5, 101)
    tr = R.toy_tower(101)
    assert native_pruned.supported(tr, x, None) is True
    tr.resblocks[1].mlp.gelu = QuickGELU()
    assert native_pruned.supported(tr, x, None) is False                                     # a QuickGELU block
    tr = R.toy_tower(101)
    tr.resblocks[2].mlp.c_fc.bias.requires_grad_(False)
    assert native_pruned.supported(tr, x, None) is False                                     # a frozen parameter, differentiated through
    with torch.no_grad():
        assert native_pruned.supported(tr, x, None) is True
    tr = R.toy_tower(101)
    tr.head_dim = 32
    assert native_pruned.supported(tr, x, None) is False                                     # heads that are not 64 wide
    tr = R.toy_tower(101)
    tr.resblocks[3].attn.head_dim = 32
    assert native_pruned.supported(tr, x, None) is False
    monkeypatch.setattr(native, "_environment_ok", lambda *a, **k: False)
    assert native_pruned.supported(R.toy_tower(101), x, None) is False


def _job(dst=0x10004, src=0x20000, rows=101, cols=509, ld_src=512, nparts=3, bf16=1, pstride=None):
    from cream_amd import _lib
    j = _lib.GradCompactJob()
    j.dst, j.src, j.ld_dst, j.ld_src = dst, src, cols, ld_src
    j.pstride = rows * ld_src if pstride is None else pstride
    j.nparts, j.rows, j.cols, j.src_bf16, j.overwrite = nparts, rows, cols, bf16, 0
    return j


def _check(jobs):
    from cream_amd import _lib
    arr = (_lib.GradCompactJob * max(1, len(jobs)))(*jobs)
    return _lib.load().cream_grad_finalize_compact_check(ctypes.cast(arr, ctypes.c_void_p), len(jobs))


def test_compact_finalize_check_on_the_host():
    """Pure host arithmetic: nothing is launched, the pointers are never read."""
    from cream_amd import _lib
    ok = [_job(dst=0x10004 + 0x100000 * i, rows=r, cols=c, ld_src=l, bf16=b)
          for i, (r, c, l, b) in enumerate([(101, 509, 512, 1), (509, 101, 104, 1), (1, 101, 104, 0), (192, 101, 104, 1), (101, 64, 64, 0),
                                            (1, 1, 8, 1), (3, 5, 8, 0), (3, 5, 12, 0)])]
    assert _check(ok) == 0 and _check([]) == 0
    bad = -1                                                                               # CREAM_ERR_BAD_ARG
    assert _check([_job(cols=509, ld_src=504)]) == bad                                    # ld_src < cols
    assert _check([_job(src=0x20008)]) == bad                                             # misaligned src
    assert _check([_job(cols=100, ld_src=100, bf16=1)]) == bad                            # ld_src % 8 != 0 with bf16 partials
    assert _check([_job(cols=100, ld_src=100, bf16=0)]) == 0                              # (fp32 partials: % 4)
    assert _check([_job(cols=101, ld_src=102, bf16=0)]) == bad
    assert _check([_job(pstride=101 * 512 + 4)]) == bad                                   # pstride % 8 != 0 with bf16 partials
    assert _check([_job(dst=0x10002)]) == bad                                             # dst not a float address
    assert _check([_job(), _job(src=0x30000)]) == bad                                     # two jobs, one dst
    assert _check([_job(dst=0x10004 + 0x100000 * i) for i in range(_lib.MAX_COMPACT_JOBS)]) == 0
    lib = _lib.load()
    arr = (_lib.GradCompactJob * (_lib.MAX_COMPACT_JOBS + 1))(*[_job(dst=0x10004 + 0x100000 * i) for i in range(_lib.MAX_COMPACT_JOBS + 1)])
    assert lib.cream_grad_finalize_compact_check(ctypes.cast(arr, ctypes.c_void_p), _lib.MAX_COMPACT_JOBS + 1) == bad
    assert lib.cream_grad_finalize_compact_check(None, 1) == bad
    assert lib.cream_grad_finalize_compact(None, 0, None) == 0                            # nothing to do: no launch
    assert lib.cream_pad_cols(None, None, _lib.F32, 0, 5, 8, None) == 0 and lib.cream_pad_cols(0x1000, 0x1000, _lib.F32, 2, 9, 8, None) == bad
    assert lib.cream_pad_cols(0x1000, 0x1000, _lib.F32, 2, 5, 6, None) == bad and lib.cream_unpad_cols(0x1000, _lib.F16, 0x1000, 2, 5, 8, None) == -2


@pytest.mark.parametrize("nparts", [1, 2, 5, 16, 17, 64, 65, 70, 300])
def test_numpy_tree_against_fp64(nparts):
    """The tree adds the nparts values of an element in at most nparts - 1 fp32 additions of non-zero operands (an addition of
    an exact zero — a lane's start, an empty lane — is exact).  Each rounds a partial sum s: |error| <= u |s| with u = 2^-24, and
    every partial sum is bounded by A = sum_p |x_p| up to the errors already made, a factor (1 + u)^(nparts - 1).  The errors
    reach the result unchanged to first order, so
        |tree - exact| <= (nparts - 1) u A (1 + u)^(nparts - 1) <= nparts u A          for nparts u << 1
    — nparts unit roundoffs of the largest partial sum in absolute values.  (nparts = 1: the value itself, error 0.)"""
    rng = np.random.default_rng(nparts)
    parts = (rng.standard_normal((nparts, 7, 33)) * np.exp(rng.standard_normal((nparts, 7, 33)))).astype(np.float32)
    got = R.tree_sum(parts)
    assert got.dtype == np.float32
    exact = parts.astype(np.float64).sum(axis=0)
    bound = nparts * 2.0 ** -24 * np.abs(parts.astype(np.float64)).sum(axis=0)
    err = np.abs(got.astype(np.float64) - exact)
    print(f"[pruned tree nparts={nparts}] worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    if nparts == 1:
        assert np.array_equal(got, parts[0])
    # the order matters and is the documented one: lane sums first
    if nparts == 5:
        p = parts
        assert np.array_equal(got, ((p[0] + p[4]) + p[1]) + p[2] + p[3])


def test_numpy_pad_unpad_roundtrip():
    x = np.arange(3 * 101, dtype=np.float32).reshape(3, 101)
    p = R.pad_cols(x, 104)
    assert p.shape == (3, 104) and np.array_equal(p[:, :101], x) and not p[:, 101:].any()
    assert np.array_equal(R.unpad_cols(p, 101), x)
    dst = np.ones((2, 5), np.float32)
    src = np.full((3, 2, 8), np.nan, np.float32)
    src[:, :, :5] = 1.0
    assert np.array_equal(R.finalize_compact(dst, src, 2, 5, 8, False), np.full((2, 5), 4.0, np.float32))
    assert np.array_equal(R.finalize_compact(dst, src, 2, 5, 8, True), np.full((2, 5), 3.0, np.float32))
