"""cream_amd/tinyvit_distill.py on the device: the sparse loss through autograd against the dense fallback, and the recipe end to
end on a toy TinyViT — one epoch of teacher logits written, read back, two student steps."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import ends_ref as E
import sparse_distill_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_tinyvit_golden import MODEL, tinyvit_fill  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hold(what, kernel, baseline, ref, floor):
    ok, uk, uf = E.check_against_fp32_baseline(kernel, baseline, ref, floor)
    print(f"\n[tinyvit_distill] {what}: kernel {uk:.2f} ulp, framework {uf:.2f} ulp", end="")
    assert ok, f"{what}: kernel error {uk:.2f} ulp of the floor's scale against the framework's {uf:.2f} ulp"


def test_sparse_loss_through_autograd_against_the_dense_fallback():
    """A (4, 21841) bf16 head output, k = 100: loss and outputs.grad (bf16, rounded once) of the kernel path against the
    float64 reference, with the dense fallback on the same tensors as the baseline — the rule of tests/test_ends_gpu.py."""
    from cream_amd import tinyvit_distill as T
    B, C, k = 4, 21841, 100
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, C, generator=g) * 3).bfloat16().to(DEV)
    index, value = R.build_records(B, C, k, 9)
    index, value = index.to(DEV), value.to(DEV)
    up = torch.tensor(0.75, device=DEV)                                        # an incoming gradient other than 1
    out_k = x.clone().requires_grad_()
    assert T.sparse_ce_supported(out_k, index, value)
    loss_k = T.sparse_soft_target_cross_entropy(out_k, index, value)
    (loss_k * up).backward()
    out_d = x.clone().requires_grad_()
    loss_d = T.dense_soft_target_cross_entropy(out_d, index, value)
    (loss_d * up).backward()
    r_rows, r_dl = R.sparse_ce(x.float(), index, value, 0.75 / B)
    assert out_k.grad.dtype == torch.bfloat16 and out_k.grad.shape == x.shape
    _hold("loss", loss_k.detach().reshape(1), loss_d.detach().reshape(1), r_rows.mean().reshape(1), floor="elem")
    _hold("outputs.grad", out_k.grad.float(), out_d.grad.float(), r_dl, floor="row")
    # outside the kernel's range the same call takes the dense formulation
    wide = torch.zeros(2, 40000, device=DEV, dtype=torch.bfloat16)
    assert not T.sparse_ce_supported(wide, index[:2], value[:2]) and not T.sparse_ce_supported(x.half(), index, value)
    assert torch.equal(T.sparse_soft_target_cross_entropy(x.half(), index, value), T.dense_soft_target_cross_entropy(x.half(), index, value))


def _toy(seed):
    from cream_amd import tinyvit
    torch.manual_seed(0)
    model = tinyvit.TinyViT(**dict(MODEL, img_size=64, num_classes=300, embed_dims=[32, 64], depths=[1, 2], num_heads=[1, 2],
                                   window_sizes=[7, 7]))
    tinyvit_fill(model, seed=seed)
    return model.to(DEV)


def test_save_logits_then_distill_on_a_toy_tinyvit(tmp_path):
    """Write one epoch of 8 synthetic frames (k = 5, 300 classes, 64 x 64), read it back, take two steps.  Replayed samples are
    bit-identical to the written pass; the stored records are the teacher's top-5; the loss of each step is finite and equals
    the same step taken with the dense fallback within 2^-7 (the bound tests/test_tinyvit_gpu.py documents for bf16 logits)."""
    from cream_amd import tinyvit_distill as T
    from cream_amd.autoformer import data as D
    from cream_amd.autoformer import engine
    k, C = 5, 300
    rng = np.random.default_rng(0)
    shapes = [(75, 100), (90, 60), (64, 64), (120, 80), (70, 70), (65, 130), (100, 100), (80, 96)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    labels = [int(v) for v in rng.integers(0, C, len(frames))]
    keys = [f"n{i // 3:02d}/img{i}.JPEG" for i in range(len(frames))]
    loader = [(frames[i:i + 4], labels[i:i + 4], keys[i:i + 4]) for i in (0, 4)]
    transform = D.DeviceTransform(64, device=DEV)
    aug = dict(reprob=0.25, auto_augment="rand-m9-mstd0.5-inc1")

    teacher = _toy(41)
    written = []

    def tap(batches):
        for item in batches:
            written.append((item[0].clone(), item[3].clone()))
            yield item

    path = T.logits_dir(str(tmp_path), k, 0)
    with T.LogitsWriter(path, rank=0) as writer:
        meters = T.save_logits_epoch(teacher, tap(T.SeededDeviceBatches(loader, transform, seed_rng=np.random.RandomState(1), **aug)),
                                     writer, k)
    assert meters["images"] == 8 and 0.0 <= meters["teacher_acc1"] <= meters["teacher_acc5"] <= 100.0
    assert os.path.getsize(os.path.join(path, "rank0-values.bin")) == 8 * T.item_size(k)

    reader = T.LogitsReader(path, k, rank=0)
    batches = list(T.SeededDeviceBatches(loader, transform, reader=reader, num_classes=C, **aug))
    reader.close()
    assert len(batches) == 2
    teacher.eval()
    for (samples, lab, index, value, seeds), (w_samples, w_seeds), (_, want_labels, _) in zip(batches, written, loader):
        assert torch.equal(samples, w_samples) and torch.equal(seeds, w_seeds) and lab.tolist() == want_labels
        assert index.dtype == torch.int16 and value.dtype == torch.float16 and index.shape == (4, k)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out = teacher(samples)
        assert np.array_equal(index.cpu().numpy().astype(np.int64), R.topk_order(out.float(), k))

    student = _toy(43)
    dense = copy.deepcopy(student)
    start = {n: v.clone() for n, v in student.state_dict().items()}
    opts = [engine.NativeAdamW(m, engine.param_groups(m), lr=1e-3) for m in (student, dense)]
    for step, batch in enumerate(batches):
        ms = T.distill_step(student, opts[0], batch, max_norm=5.0)
        md = T.distill_step(dense, opts[1], batch, max_norm=5.0, criterion=T.dense_soft_target_cross_entropy)
        print(f"\n[tinyvit_distill] step {step}: loss {ms['loss']:.6f}  dense fallback {md['loss']:.6f}", end="")
        assert np.isfinite(ms["loss"]) and abs(ms["loss"] - md["loss"]) <= 2.0 ** -7 * abs(md["loss"])
        assert set(ms) == {"loss", "train_acc1", "train_acc5", "teacher_acc1", "teacher_acc5"}
        assert ms["teacher_acc1"] == md["teacher_acc1"] and 0.0 <= ms["teacher_acc1"] <= ms["teacher_acc5"] <= 100.0
    moved = max(float((v.float() - start[n].float()).abs().max()) for n, v in student.state_dict().items())
    assert moved > 0 and all(bool(torch.isfinite(p).all()) for p in student.parameters())
