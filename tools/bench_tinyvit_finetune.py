#!/usr/bin/env python
"""TinyViT's fine-tune step (cream_amd/tinyvit_finetune.py) with the layer-wise learning-rate decay of the 22k -> 1k and
higher-resolution recipes (layer_lr_decay 0.8, clip 5.0, weight decay 1e-8, BatchNorm in eval mode, bf16 autocast):
`NativeAdamW` — per-group rates and the clip inside ONE launch — against torch.optim.AdamW(fused=True) on the same groups plus
torch's clip_grad_norm_.  Same process, same model, same data, runs interleaved.

    python tools/bench_tinyvit_finetune.py [--reps 20] [--warmup 3] [--out FILE]

Per model (tiny_vit_21m_224 at B = 128; tiny_vit_21m_384 at the largest batch up to 64 that fits) three JSON lines:
  part "step"       the whole finetune_step, either optimizer
  part "optimizer"  clip + update alone on given gradients
  part "launch"     cream_adamw_step_groups against cream_adamw_step on the SAME job table, every group at the same rate
each with the median ms, the run-to-run spread (half the inter-quartile range as a fraction of the median) and the ratio."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tinyvit import interleaved  # noqa: E402

LR = 1e-6                                  # small: hundreds of timed updates must leave the weights where they are


def bench_model(name, size, B, reps, warmup):
    from cream_amd import tinyvit
    from cream_amd import tinyvit_finetune as FT
    from cream_amd.autoformer.engine import NativeAdamW
    torch.manual_seed(0)
    model = getattr(tinyvit, name)(layer_lr_decay=0.8).cuda()
    x = torch.randn(B, 3, size, size, device="cuda")
    y = torch.randint(0, 1000, (B,), device="cuda")
    native = FT.build_finetune_optimizer(model, LR)
    assert isinstance(native, NativeAdamW)
    fused = torch.optim.AdamW(FT.finetune_param_groups(model), lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-8, fused=True)
    for opt in (native, fused):
        for g in opt.param_groups:
            g['lr'] = LR * g['lr_scale']
    base = dict(model=name, B=B, groups=len(native.param_groups), rates=len({g['lr'] for g in native.param_groups}))

    # the whole step
    def step(opt):
        def f():
            FT.finetune_step(model, opt, x, y, max_norm=5.0)
        return f

    model.zero_grad(set_to_none=True)
    r = interleaved({"native": step(native), "torch_fused": step(fused)}, reps, warmup)
    r["ratio"] = round(r["torch_fused_ms"] / r["native_ms"], 3)
    yield dict(base, part="step", **r)

    # clip + update alone
    for p in model.parameters():
        p.grad = torch.randn_like(p) * 1e-2

    def native_update():
        native.step(max_norm=5.0)

    def torch_update():
        torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
        fused.step()

    r = interleaved({"native": native_update, "torch_fused": torch_update}, 4 * reps, warmup)
    r["ratio"] = round(r["torch_fused_ms"] / r["native_ms"], 3)
    yield dict(base, part="optimizer", **r)

    # the two launches on one table, all groups at one rate
    table, n, k = native._table, len(native.param_groups), [native._steps]

    def launch(lr):
        def f():
            k[0] += 1
            table.launch(update=True, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, step=k[0])
        return f

    r = interleaved({"grouped": launch([LR] * n), "ungrouped": launch(LR)}, 8 * reps, warmup)
    r["ratio"] = round(r["grouped_ms"] / r["ungrouped_ms"], 4)
    r["within_spreads"] = bool(r["grouped_ms"] - r["ungrouped_ms"] <= (r["grouped_spread"] + r["ungrouped_spread"]) * r["ungrouped_ms"])
    yield dict(base, part="launch", jobs=table.n, tiles=table.total, **r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about speed"

    def emit(r):
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    for r in bench_model("tiny_vit_21m_224", 224, 128, a.reps, a.warmup):
        emit(r)
    B = 64
    while B >= 1:                                                  # the largest batch up to 64 that fits
        try:
            for r in bench_model("tiny_vit_21m_384", 384, B, a.reps, a.warmup):
                emit(r)
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            emit(dict(model="tiny_vit_21m_384", B=B, out_of_memory=True))
            B //= 2


if __name__ == "__main__":
    main()
