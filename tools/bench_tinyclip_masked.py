#!/usr/bin/env python
"""TinyCLIP's mask-learning step (automatic weight inheritance) on one device: the STUDENT step of BASELINE config 5's model
(TinyCLIP-ViT-39M-16-Text-19M, 256 pairs, bf16 autocast; the frozen teacher's features are computed once outside the timed
region: they are the same in every mode) in three modes, one process, one call, runs interleaved:

    dense      masks off, the native tower node — the code of the dense recipe, unchanged
    composed   both l0 modules, the composed masked path (CREAM_TINYCLIP_NATIVE=0's route: module by module, the masks as
               element-wise multiplications, the masked LayerNorm as index_select / layer_norm / scatter)
    native     both l0 modules, the masked native node (cream_amd/tinyclip/native_masked.py)

    python tools/bench_tinyclip_masked.py [--reps 20] [--warmup 4] [--batch 256] [--out FILE]
    python tools/bench_tinyclip_masked.py --only native --reps 5          (the run to put under a kernel trace)

One JSON line per part: `student_step` (median ms per mode, spread = half the inter-quartile range over the median, the
ratios native / dense and composed / native, the new launches' time regions with bytes counted from shapes) and
`masked_block` (forward + backward of ONE masked block of the image tower's shape, composed and native)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REGIONS = ("ln_fwd_masked", "ln_bwd_masked", "mask_pack", "mask_grad_finalize")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def interleaved(steps, reps, warmup):
    """steps {name: fn} -> {name_ms, name_spread}: two rounds over the modes, so that drift hits all of them."""
    half = max(reps // 2, 2)
    runs, out = {k: [] for k in steps}, {}
    for _ in range(2):
        for name, fn in steps.items():
            runs[name] += timed(fn, half, warmup)
    for name in steps:
        q = statistics.quantiles(runs[name], n=4)
        med = statistics.median(runs[name])
        out[name + "_ms"], out[name + "_spread"] = round(med, 3), round(0.5 * (q[2] - q[0]) / med, 4)
    return out


def spread_logas(l0, seed):
    """Log-alphas around 0 (N(0, 3)): the sampled masks hold exact zeros, as in the middle of a pruning run."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in l0.z_logas.values():
            p.copy_(3.0 * torch.randn(p.shape, generator=g))


def student_steps(batch, only):
    """-> {mode: fn}: one student step per call (forward, soft loss + Lagrangian term, backward, clip, both optimizers)."""
    import cream_amd.tinyclip.model as M
    from cream_amd.tinyclip import distill
    dev = torch.device("cuda")
    torch.manual_seed(0)
    teacher = M.create_model("ViT-B-16").to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    images = torch.randn(batch, 3, 224, 224, device=dev, generator=g)
    texts = torch.randint(1, 49406, (batch, 77), device=dev, generator=g)
    texts[:, 40] = 49407                                        # end-of-text
    texts[:, 41:] = 0
    steps, cached = {}, None

    def make(masked, native_on):
        nonlocal cached
        torch.manual_seed(1)
        student = M.create_model("TinyCLIP-ViT-39M-16-Text-19M", mask_image=masked, mask_text=masked,
                                 mask_cfg=dict(sparsity_warmup=1000, sparsity=0.5, start_sparsity=0.0)).to(dev)
        l0_opt = None
        if masked:
            spread_logas(student._image_encoder.l0_module, 5)
            spread_logas(student._text_encoder.l0_module, 9)
            l0_opt = distill.make_l0_optimizer(student)
        opt = torch.optim.AdamW(distill.student_parameters(student), lr=1e-4, weight_decay=0.2, fused=True)
        step = distill.DistillStep(student, teacher, opt, logit_scale=50.0, norm_gradient_clip=5.0, amp_dtype=torch.bfloat16,
                                   l0_optimizer=l0_opt, total_loss_flag=True)
        if cached is None:
            cached = step.teacher_outputs(images, texts)
        step.teacher_outputs = lambda *_: cached                # the frozen teacher: outside the student step

        def f():
            M.NATIVE_TOWERS = native_on
            try:
                step.step(images, texts)
            finally:
                M.NATIVE_TOWERS = True
        return f

    for name, (masked, native_on) in dict(dense=(False, True), composed=(True, False), native=(True, True)).items():
        if only in (None, name):
            steps[name] = make(masked, native_on)
    del teacher
    return steps


def masked_block(batch, reps, warmup):
    """Forward + backward of one masked block of the image tower's shape (D 512, 8 heads, F 2048, L 197)."""
    import cream_amd.tinyclip.model as M
    torch.manual_seed(2)
    tr = M.Transformer(512, 1, 8).cuda()
    g = torch.Generator().manual_seed(3)
    zh, zd, zi = (torch.rand(n, generator=g) for n in (512, 8, 2048))
    zh[torch.rand(512, generator=g) < 0.3] = 0
    zd[3] = 0
    zi[torch.rand(2048, generator=g) < 0.3] = 0
    zh, zd, zi = (z.cuda().requires_grad_() for z in (zh, zd, zi))
    x = torch.randn(batch, 197, 512, device="cuda", requires_grad=True)
    gy = torch.randn(batch, 197, 512, device="cuda")

    def run(native_on):
        def f():
            M.NATIVE_TOWERS = native_on
            try:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = tr(x, hidden_z=zh, heads_z=zd.view(1, 8), intermediate_z=zi.view(1, -1))
                y.float().backward(gy)
            finally:
                M.NATIVE_TOWERS = True
        return f

    r = interleaved({"composed": run(False), "native": run(True)}, reps, warmup)
    r["composed_over_native"] = round(r["composed_ms"] / r["native_ms"], 3)
    return dict(part="masked_block", shape=dict(B=batch, L=197, D=512, H=8, F=2048), **r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", choices=("dense", "composed", "native"), default=None, help="one mode alone (a run under a kernel trace)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about speed"
    from cream_amd import timing

    def emit(r):
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    steps = student_steps(a.batch, a.only)
    r = interleaved(steps, a.reps, a.warmup)
    if a.only is None:
        r["native_over_dense"] = round(r["native_ms"] / r["dense_ms"], 3)
        r["composed_over_native"] = round(r["composed_ms"] / r["native_ms"], 3)
    if "native" in steps:
        timing.reset()
        timing.enable(True, only=REGIONS)
        for _ in range(3):
            steps["native"]()
        timing.enable(False)
        r["regions_per_step"] = {k: dict(launches=v["launches"] // 3, ms=round(v["total_ms"] / 3, 3),
                                         gb_s=round(v["bytes"] / (v["total_ms"] * 1e-3) / 1e9, 1) if v["total_ms"] > 0 else None)
                                 for k, v in sorted(timing.summary().items())}
        timing.reset()
    emit(dict(part="student_step", model="TinyCLIP-ViT-39M-16-Text-19M", batch=a.batch, **r))
    if a.only is None:
        emit(masked_block(a.batch, a.reps, a.warmup))


if __name__ == "__main__":
    main()
