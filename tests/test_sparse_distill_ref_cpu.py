"""The float64 references of tests/sparse_distill_ref.py against the framework's own float64 operators, the order rule
against torch.topk on the builder's inputs, and the torch fallbacks of cream_amd/tinyvit_distill.py against the reference's
formulation (TinyViT/main.py:321-330, TinyViT/save_logits.py:135-157) written out step by step.  No device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_distill_ref as R


def _case(B, C, k, seed, total=0.9):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, C, generator=g, dtype=torch.float64) * 2 - 1) * 20
    index, value = R.build_records(B, C, k, seed + 1, total)
    return x, index, value


@pytest.mark.parametrize("C,k,total", [(6, 5, 0.9), (257, 5, 0.9), (257, 128, 1.002), (1000, 100, 0.5), (21841, 100, 0.9)])
def test_reference_loss_is_soft_target_ce_over_the_recovered_teacher(C, k, total):
    from cream_amd.tinyvit_distill import recover_teacher
    x, index, value = _case(3, C, k, C + k, total)
    xr = x.clone().requires_grad_()
    # recover_teacher works in fp32 as the reference does; the float64 teacher is rebuilt from the same record here
    teacher = R.dense_target(index, value, C)
    assert torch.allclose(recover_teacher(index, value, C).double(), teacher, rtol=1e-6, atol=1e-9)
    rows = torch.sum(-teacher * F.log_softmax(xr, dim=-1), dim=-1)
    (gx,) = torch.autograd.grad(rows.sum() * 0.25, xr)
    loss, dl = R.sparse_ce(x, index, value, 0.25)
    torch.testing.assert_close(loss, rows.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(dl, gx, rtol=1e-11, atol=1e-16)
    if total > 1:
        assert float(teacher.min()) < 0                     # the case with `minor` < 0 is one


@pytest.mark.parametrize("C,k", [(6, 5), (257, 65), (21841, 100), (32768, 128)])
def test_closed_form_of_the_kernel_header_equals_the_dense_reference(C, k):
    x, index, value = _case(2, C, k, 3 * C + k)
    loss, _ = R.sparse_ce(x, index, value, 1.0)
    torch.testing.assert_close(R.sparse_ce_closed_form(x, index, value), loss, rtol=1e-12, atol=0)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,k", [(21841, 100), (1000, 100), (130, 128), (32768, 128), (257, 5)])
def test_order_rule_agrees_with_torch_topk_on_the_builders_inputs(C, k, dt):
    x = R.build_topk_logits(2, C, k, C + k).to(dt)
    got = torch.softmax(x.float(), -1).topk(k, dim=-1, largest=True, sorted=True).indices
    assert np.array_equal(got.numpy(), R.topk_order(x.float(), k))


def test_order_rule_breaks_ties_by_ascending_class():
    x = torch.tensor([[1.0, 3.0, 3.0, -1.0, 3.0, 1.0]])
    assert R.topk_order(x, 5).tolist() == [[1, 2, 4, 0, 5]]


def test_fp16_value_rule():
    r = np.array([0.1, 2.0 ** -20, 2.0 ** -20, 0.0])
    h = np.array([0.1, 2.0 ** -20, 0.0, 0.0], dtype=np.float16)
    assert R.fp16_value_ok(h, r, 1e-6).tolist() == [True, True, False, True]
    assert not R.fp16_value_ok(np.float16(0.1) + np.float16(2.0 ** -13), np.array(0.1), 1e-6)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float64])
def test_loss_fallback_is_the_reference_formulation(dt):
    from cream_amd import tinyvit_distill as T
    C, k = 301, 7
    x, index, value = _case(4, C, k, 11)
    outputs = x.to(dt).requires_grad_()
    assert not T.sparse_ce_supported(outputs, index, value)
    loss = T.sparse_soft_target_cross_entropy(outputs, index, value)
    # main.py:321-330, one step at a time
    li, lv = index.long(), value.float()
    minor = (1.0 - lv.sum(-1, keepdim=True)) / (C - k)
    teacher = minor.repeat_interleave(C, dim=-1)
    teacher.scatter_(-1, li, lv)
    ref_in = outputs.detach().clone().requires_grad_()
    ref = torch.sum(-teacher * F.log_softmax(ref_in.float(), dim=-1), dim=-1).mean()
    assert torch.equal(loss, ref) and torch.equal(T.recover_teacher(index, value, C), teacher)
    loss.backward()
    ref.backward()
    assert torch.equal(outputs.grad, ref_in.grad)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_records_fallback_is_the_reference_formulation(dt):
    from cream_amd import tinyvit_distill as T
    k = 5
    outputs = R.build_topk_logits(3, 40, k, 5).to(dt)
    seeds = torch.tensor([7, 2 ** 31 - 1, 0], dtype=torch.int32)
    rec = T.topk_records(outputs, seeds, k)
    assert rec.dtype == torch.uint8 and rec.shape == (3, 4 + 4 * k)
    # save_logits.py:135-157
    values, indices = torch.softmax(outputs.float(), -1).topk(k=k, dim=-1, largest=True, sorted=True)
    values, indices = values.to(torch.float16).numpy(), indices.to(torch.int16).numpy()
    for row, seed, ind, val in zip(rec.numpy(), seeds.numpy(), indices, values):
        assert row.tobytes() == seed.tobytes() + ind.tobytes() + val.tobytes()
    assert np.array_equal(rec.numpy(), T.pack_records(seeds.numpy(), indices, values))
