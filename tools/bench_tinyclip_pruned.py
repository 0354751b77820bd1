#!/usr/bin/env python
"""The distillation step of a PRUNED TinyCLIP student on one device: BASELINE config 5's student
(TinyCLIP-ViT-39M-16-Text-19M, 256 pairs, bf16 autocast) with both l0 modules, log-alphas drawn as in
tools/bench_tinyclip_masked.py, the deterministic masks rounded to 0 / 1, `fuse_masks` — then the student step (the frozen
teacher's features are computed once outside the timed region) in three modes, one process, one call, runs interleaved:

    pruned_native     the pruned student, its towers on cream_amd/tinyclip/native_pruned.py (padded operands)
    pruned_composed   the same student module by module through the framework (CREAM_TINYCLIP_NATIVE=0's route)
    dense             the unpruned dense student on the native tower node — the code of the dense recipe

    python tools/bench_tinyclip_pruned.py [--reps 20] [--warmup 4] [--batch 256] [--out FILE]
    python tools/bench_tinyclip_pruned.py --only pruned_native --reps 5          (the run to put under a kernel trace)

One JSON line: the pruned shapes (d, H_l, F_l per tower), median ms per mode with spread = half the inter-quartile range over
the median, the ratios pruned_composed / pruned_native and pruned_native / dense, and the new launches' time regions."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tinyclip_masked import interleaved, spread_logas  # noqa: E402

MODES = ("pruned_native", "pruned_composed", "dense")
REGIONS = ("pad_cols", "unpad_cols", "grad_finalize_compact", "ln_fwd_masked", "ln_bwd_masked")


def binary_masks(student):
    """The deterministic masks rounded to 0 / 1: a log-alpha above 0 keeps its unit, the others are cut."""
    with torch.no_grad():
        for enc in (student._image_encoder, student._text_encoder):
            for p in enc.l0_module.z_logas.values():
                p.copy_(torch.where(p > 0, torch.full_like(p, 40.0), torch.full_like(p, -40.0)))


def student_steps(batch, only):
    """-> ({mode: fn}, pruned shapes): one student step per call (forward, soft loss, backward, clip, optimizer)."""
    import cream_amd.tinyclip.model as M
    from cream_amd.tinyclip import distill, native_pruned
    dev = torch.device("cuda")
    torch.manual_seed(0)
    teacher = M.create_model("ViT-B-16").to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    images = torch.randn(batch, 3, 224, 224, device=dev, generator=g)
    texts = torch.randint(1, 49406, (batch, 77), device=dev, generator=g)
    texts[:, 40] = 49407                                        # end-of-text
    texts[:, 41:] = 0
    cached = None

    def stepper(student):
        nonlocal cached
        opt = torch.optim.AdamW(distill.student_parameters(student), lr=1e-4, weight_decay=0.2, fused=True)
        step = distill.DistillStep(student, teacher, opt, logit_scale=50.0, norm_gradient_clip=5.0, amp_dtype=torch.bfloat16)
        if cached is None:
            cached = step.teacher_outputs(images, texts)
        step.teacher_outputs = lambda *_: cached                # the frozen teacher: outside the student step
        return step

    def mode(step, native_on):
        def f():
            M.NATIVE_TOWERS = native_on
            try:
                step.step(images, texts)
            finally:
                M.NATIVE_TOWERS = True
        return f

    steps, shapes = {}, {}
    if only in (None, "pruned_native", "pruned_composed"):
        torch.manual_seed(1)
        student = M.create_model("TinyCLIP-ViT-39M-16-Text-19M", mask_image=True, mask_text=True,
                                 mask_cfg=dict(sparsity_warmup=1000, sparsity=0.5, start_sparsity=0.0)).to(dev)
        spread_logas(student._image_encoder.l0_module, 5)
        spread_logas(student._text_encoder.l0_module, 9)
        binary_masks(student)
        distill.fuse_masks(student, images[:1], texts[:1])
        student.train()
        for name, tr in (("image", student._image_encoder.visual.transformer), ("text", student._text_encoder.transformer)):
            pl = native_pruned.plan(tr)
            shapes[name] = dict(d=pl["d"], Dp=pl["Dp"], H=[b["H"] for b in pl["blocks"]], F=[b["F"] for b in pl["blocks"]])
        shapes["parameters"] = sum(p.numel() for p in student.parameters())
        step = stepper(student)
        for name, native_on in (("pruned_native", True), ("pruned_composed", False)):
            if only in (None, name):
                steps[name] = mode(step, native_on)
    if only in (None, "dense"):
        torch.manual_seed(1)
        dense = M.create_model("TinyCLIP-ViT-39M-16-Text-19M").to(dev)
        shapes["dense_parameters"] = sum(p.numel() for p in dense.parameters())
        steps["dense"] = mode(stepper(dense), True)
    return steps, shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", choices=MODES, default=None, help="one mode alone (a run under a kernel trace)")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about speed"
    from cream_amd import timing
    steps, shapes = student_steps(a.batch, a.only)
    print(json.dumps(dict(part="pruned_shapes", **shapes)), flush=True)
    r = interleaved(steps, a.reps, a.warmup)
    if a.only is None:
        r["composed_over_native"] = round(r["pruned_composed_ms"] / r["pruned_native_ms"], 3)
        r["native_over_dense"] = round(r["pruned_native_ms"] / r["dense_ms"], 3)
    if "pruned_native" in steps:
        timing.reset()
        timing.enable(True, only=REGIONS)
        for _ in range(3):
            steps["pruned_native"]()
        timing.enable(False)
        r["regions_per_step"] = {k: dict(launches=v["launches"] // 3, ms=round(v["total_ms"] / 3, 3)) for k, v in sorted(timing.summary().items())}
        timing.reset()
    out = dict(part="student_step", model="TinyCLIP-ViT-39M-16-Text-19M (pruned by 0 / 1 masks, fuse_masks)", batch=a.batch, shapes=shapes, **r)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
