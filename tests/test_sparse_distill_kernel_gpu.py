"""Kernel-level parity of csrc/sparse_distill.hip (cream_sparse_ce, cream_softmax_topk_records) against the float64 references
of tests/sparse_distill_ref.py, through the C ABI on tiny tensors, with the conventions of tests/test_ends_gpu.py: outputs are
prefilled with NaN (records with a sentinel byte), every output has a sentinel band behind it that must survive, and fp32 sums
and transcendental functions are held to ends_ref.check_against_fp32_baseline (margin 4 over the framework's own fp32 error
plus a floor of 4 fp32 ulp) — no tolerance of this file's own.

Shapes: C in {k + 1, 255, 256, 257, 1000, 2049, 21841, 32768}, each with k = 5 and with k = 100 or 128; every k in
{1, 5, 63, 64, 65, 100, 128} at C = 257 and C = 21841; B = 1 or 3; both logit dtypes.  Where C is odd the logits start one
element behind a 16-byte boundary, so every row sits at an odd element offset (2-byte alignment in bf16)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ends_ref as E
import sparse_distill_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -1984.0
BAND = 64
OK, BAD_ARG, BAD_DTYPE, TOO_LARGE = 0, -1, -2, -4
NAN = float("nan")
KS = (1, 5, 63, 64, 65, 100, 128)
CASES = sorted({(C, 5) for C in (6, 255, 256, 257, 1000, 2049, 21841, 32768)} |
               {(101, 100), (255, 100), (257, 100), (1000, 100), (21841, 100)} |
               {(129, 128), (256, 128), (2049, 128), (32768, 128)} |
               {(C, k) for C in (257, 21841) for k in KS})


def _lib():
    from cream_amd import _lib as L
    return L.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """A buffer of `shape` (prefilled with `fill`) with BAND sentinel elements behind it; .t is the 16-byte aligned view."""

    def __init__(self, shape, dtype=torch.float32, fill=NAN, sent=SENT):
        self.n, self.sent = math.prod(shape), sent
        self.whole = torch.full((self.n + BAND,), sent, dtype=dtype, device=DEV)
        self.t = self.whole[:self.n].view(shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.whole[self.n:] == self.sent).all())


def _place(x, dt):
    """x (B, C) fp32 on the host -> device tensor of dtype dt, contiguous; for odd C one element behind a 16-byte boundary."""
    B, C = x.shape
    off = C % 2
    flat = torch.zeros(B * C + off, dtype=dt, device=DEV)
    out = flat[off:].view(B, C)
    out.copy_(x.to(DEV))
    assert out.data_ptr() % 16 == off * out.element_size()
    return out


def _hold(what, kernel, baseline, ref, floor):
    ok, uk, uf = E.check_against_fp32_baseline(kernel, baseline, ref, floor)
    print(f"\n[sparse_distill] {what}: kernel {uk:.2f} ulp, framework fp32 {uf:.2f} ulp", end="")
    assert ok, f"{what}: kernel error {uk:.2f} ulp of the floor's scale against framework fp32 {uf:.2f} ulp"


# ---- cream_sparse_ce --------------------------------------------------------------------------------------------------------
def _ce_run(lib, logits, index, value, gs):
    B, C = logits.shape
    code = 2 if logits.dtype == torch.bfloat16 else 0
    rows, dl = Guarded((B,)), Guarded((B, C))
    assert lib.cream_sparse_ce(_p(rows.t), _p(dl.t), _p(logits), _p(index), _p(value), B, C, index.shape[1], code, gs, _stream()) == OK
    torch.cuda.synchronize()
    assert rows.intact() and dl.intact(), "sentinel band overwritten"
    assert bool(torch.isfinite(rows.t).all()) and bool(torch.isfinite(dl.t).all())
    return rows.t, dl.t


def _ce_framework(x32, index, value, gs):
    """The reference's dense formulation (TinyViT/main.py:321-330) in fp32 on the device, gradient by autograd."""
    C = x32.shape[1]
    lv = value.float()
    minor = (1.0 - lv.sum(-1, keepdim=True)) / (C - index.shape[1])
    teacher = minor.repeat_interleave(C, dim=-1).scatter_(-1, index.long(), lv)
    xr = x32.clone().requires_grad_()
    rows = torch.sum(-teacher * torch.log_softmax(xr, -1), -1)
    (gx,) = torch.autograd.grad(rows.sum() * gs, xr)
    return rows.detach(), gx


def _ce_case(C, k, dt, B, total):
    amp = 80.0 if dt == torch.float32 else 60.0
    g = torch.Generator().manual_seed(C * 131 + k + (7 if dt == torch.float32 else 13))
    x = (torch.rand(B, C, generator=g) * 2 - 1) * amp
    x[:, 0] = amp
    x[:, C // 2] = -amp
    logits = _place(x, dt)
    index, value = R.build_records(B, C, k, C + 17 * k, total)
    index, value = index.to(DEV), value.to(DEV)
    gs = 1.0 / B
    rows, dl = _ce_run(_lib(), logits, index, value, gs)
    x32 = logits.float()
    r_rows, r_dl = R.sparse_ce(x32, index, value, gs)
    fw_rows, fw_dl = _ce_framework(x32, index, value, gs)
    tag = f"C={C} k={k} B={B} {str(dt)[6:]} sum={total}"
    _hold(f"sparse_ce loss @ {tag}", rows, fw_rows, r_rows, floor="elem")
    _hold(f"sparse_ce dlogits @ {tag}", dl, fw_dl, r_dl, floor="row")
    return value


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,k", CASES)
def test_sparse_ce_against_float64_at_large_logits(C, k, dt):
    """Loss rows (floor "elem") and the dense gradient (floor "row") with logits spread over +-80 (fp32) / +-60 (bf16); the
    framework's fp32 run of the dense formulation is the baseline.  C = k + 1 is the case with a single unpatched class.
    Measured on the MI355X (worst over the cases and both dtypes): loss rows kernel 2.22 ulp / framework fp32 1.86 ulp of the
    value, dlogits 1.83 / 2.25 ulp of the row's largest gradient."""
    _ce_case(C, k, dt, B=1 if (C + k) % 4 == 0 else 3, total=0.9)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,k", [(257, 5), (21841, 100)])
def test_sparse_ce_with_values_summing_above_one(C, k, dt):
    """fp16 values that sum above 1: `minor` is negative, the loss has terms of both signs."""
    value = _ce_case(C, k, dt, B=3, total=1.002)
    assert float(value.float().sum(-1).min()) > 1.0


def test_sparse_ce_refuses_bad_arguments_without_launching():
    lib = _lib()
    B, C, k = 2, 300, 5
    rows, dl = Guarded((B,)), Guarded((B, C))
    x = torch.zeros(B, 40000, device=DEV)
    index = torch.zeros(B, 200, dtype=torch.int16, device=DEV)
    value = torch.zeros(B, 200, dtype=torch.float16, device=DEV)
    call = lambda *a: lib.cream_sparse_ce(*a, _stream())          # noqa: E731
    assert call(_p(rows.t), _p(dl.t), _p(x), _p(index), _p(value), B, C, 129, 0, 1.0) == TOO_LARGE
    assert call(_p(rows.t), _p(dl.t), _p(x), _p(index), _p(value), B, 32769, k, 0, 1.0) == TOO_LARGE
    for kk in (100, 101, 0, -1):                                   # k >= C, k < 1
        assert call(_p(rows.t), _p(dl.t), _p(x), _p(index), _p(value), B, 100, kk, 0, 1.0) == BAD_ARG
    for i in range(5):
        args = [_p(rows.t), _p(dl.t), _p(x), _p(index), _p(value)]
        args[i] = None
        assert call(*args, B, C, k, 0, 1.0) == BAD_ARG
    for code in (1, 3, 7):
        assert call(_p(rows.t), _p(dl.t), _p(x), _p(index), _p(value), B, C, k, code, 1.0) == BAD_DTYPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(rows.t).all()) and bool(torch.isnan(dl.t).all()) and rows.intact() and dl.intact()


# ---- cream_softmax_topk_records ---------------------------------------------------------------------------------------------
REC_SENT = 0xA5


def _records_run(lib, logits, seeds, k):
    B, C = logits.shape
    code = 2 if logits.dtype == torch.bfloat16 else 0
    rec = Guarded((B, 4 + 4 * k), dtype=torch.uint8, fill=REC_SENT, sent=0x5A)
    assert lib.cream_softmax_topk_records(_p(rec.t), _p(logits), _p(seeds), B, C, k, code, _stream()) == OK
    torch.cuda.synchronize()
    assert rec.intact(), "sentinel band overwritten"
    return rec.t.cpu().numpy()


def _records_check(x, dt, k, seed, check_values=True):
    """Runs the kernel on x (host fp32, exact in dt) and checks indices (exactly the order rule), values (the fp16 rule),
    seeds and the record bytes.  -> (index, value, fp64 probabilities of the chosen classes)."""
    from cream_amd.tinyvit_distill import pack_records
    B, C = x.shape
    logits = _place(x, dt)
    g = torch.Generator().manual_seed(seed)
    seeds = torch.randint(0, 2 ** 31 - 1, (B,), generator=g, dtype=torch.int64).to(torch.int32)
    seeds[0] = 2 ** 31 - 1
    rec = _records_run(_lib(), logits, seeds.to(DEV), k)
    got_seed = rec[:, :4].copy().view(np.int32).reshape(-1)
    index = rec[:, 4:4 + 2 * k].copy().view(np.int16)
    value = rec[:, 4 + 2 * k:].copy().view(np.float16)
    assert np.array_equal(got_seed, seeds.numpy())
    want = R.topk_order(logits.float(), k)
    assert np.array_equal(index.astype(np.int64), want), "indices differ from the order rule"
    p64 = R.softmax64(logits.float())
    p32 = torch.softmax(logits.float(), -1)
    chosen = torch.gather(p64, 1, torch.from_numpy(want).to(DEV)).cpu().numpy()
    if check_values:
        rel = ((p32.double() - p64).abs() / p64).amax(-1).cpu().numpy()              # the framework's fp32 softmax, per row
        eps = 4 * rel + 4 * E.ULP32
        ok = R.fp16_value_ok(value, chosen, eps[:, None])
        print(f"\n[sparse_distill] records C={C} k={k} {str(dt)[6:]}: framework fp32 softmax rel err {rel.max():.2e}, "
              f"eps {eps.max():.2e}, smallest value {float(value.min()):.3e}", end="")
        assert ok.all(), f"{int((~ok).sum())} fp16 values are not the rounding of a real within eps of the float64 softmax"
    # byte for byte: the record is pack_records of the checked pieces
    assert np.array_equal(rec, pack_records(got_seed, index, value))
    return index, value, chosen


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,k", CASES)
def test_topk_records_indices_values_and_bytes(C, k, dt):
    """Distinct top k + 1 logits (the builder), ties below them: indices equal the order rule, values obey the fp16 rule."""
    B = 1 if (C + k) % 4 == 0 else 3
    _records_check(R.build_topk_logits(B, C, k, 7 * C + k), dt, k, C + k)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_topk_records_keep_fp16_subnormals(dt):
    """Top logits 6 - j / 8, k = 100: the tail of the record lies below 2^-14 and above 2^-24.  A flush to zero fails."""
    C, k = 1000, 100
    _, value, chosen = _records_check(R.build_topk_logits(3, C, k, 99, step=1.0 / 8), dt, k, 5)
    sub = (chosen < 2.0 ** -14) & (chosen > 2.0 ** -23)
    assert sub.sum() >= 3 * 10 and (value[sub] > 0).all() and (value[sub].astype(np.float64) <= 2.0 ** -14).all()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,k", [(6, 5), (257, 5), (257, 128), (1000, 100), (2049, 65), (21841, 100), (32768, 128), (128, 128)])
def test_topk_records_heavy_ties_go_by_ascending_class(C, k, dt):
    """Logits drawn from 7 distinct values: the k-th value is shared by many classes inside and outside the record.  Indices
    are held to the stable-argsort rule alone (torch.topk leaves ties open and is not consulted); values as everywhere."""
    g = torch.Generator().manual_seed(C + k)
    x = (torch.randint(0, 7, (3, C), generator=g).float() - 3) * 0.5
    x[1, : C // 2] = 0.0                                    # one row with a signed zero among its ties
    x[1, 0] = -0.0
    _records_check(x, dt, k, 3 * C + k)


def test_topk_records_refuses_bad_arguments_without_launching():
    lib = _lib()
    B, C, k = 2, 300, 5
    rec = Guarded((B, 4 + 4 * 128), dtype=torch.uint8, fill=REC_SENT, sent=0x5A)
    x = torch.zeros(B, 40000, device=DEV)
    seeds = torch.zeros(B, dtype=torch.int32, device=DEV)
    call = lambda *a: lib.cream_softmax_topk_records(*a, _stream())          # noqa: E731
    assert call(_p(rec.t), _p(x), _p(seeds), B, C, 129, 0) == TOO_LARGE
    assert call(_p(rec.t), _p(x), _p(seeds), B, 32769, k, 0) == TOO_LARGE
    assert call(_p(rec.t), _p(x), _p(seeds), B, 100, 101, 0) == BAD_ARG
    assert call(_p(rec.t), _p(x), _p(seeds), B, C, 0, 0) == BAD_ARG
    for i in range(3):
        args = [_p(rec.t), _p(x), _p(seeds)]
        args[i] = None
        assert call(*args, B, C, k, 0) == BAD_ARG
    for code in (1, 3, 7):
        assert call(_p(rec.t), _p(x), _p(seeds), B, C, k, code) == BAD_DTYPE
    torch.cuda.synchronize()
    assert bool((rec.t == REC_SENT).all()) and rec.intact()
