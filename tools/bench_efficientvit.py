#!/usr/bin/env python
"""EfficientViT's attention layer (`LocalWindowAttention`) at the three stage shapes of M0, M4 and M5, eval mode at B = 128
under bf16 autocast and `torch.no_grad()`: the fused cascaded group attention (cream_amd/cga_attn.py) against the composed
branch of the same code, same process, same data, runs interleaved.

    python tools/bench_efficientvit.py [--reps 30] [--warmup 5] [--pairs] [--split] [--models] [--skip-layers] [--out FILE]

Per stage shape it prints one JSON line: median ms of each path, the run-to-run spread (half the inter-quartile range as a
fraction of the median), the ratio composed / fused, and the kernel alone (the timing region's events around the launch) with
its FLOP/s counted from shapes.  The layer's input is the contiguous NCHW bf16 tensor the preceding FFN hands it, so the fused
path's transposition into the token layout is inside the measurement.  Composed means CREAM_IRPE_FUSED=0.

--models adds whole-model evaluation by the protocol of EfficientViT/classification/speed_test.py: BatchNorm fused
(`replace_batchnorm`), autocast, batch 2048 at 224 x 224, images/s from the mean time of synchronised calls — here under
`torch.no_grad()` and without `torch.jit.trace` (the fused path is a C call), with three paths interleaved: tokens (the default:
the map stays (B, H, W, C) and every dw + FFN pair is one launch of cream_amd/evit_ffn.py), parent (`fused_blocks=False`: the
fused attention alone) and composed.

--pairs adds the depthwise 3 x 3 + FFN pair of every stage shape at B = --batch and --model-batch, one launch against the
composed pair, with the bytes counted from shapes (x in, y out, the weights once) as a fraction of the 6.29 TB/s copy rate.
--split adds the parent path's time per part of the model (stem, pairs, mixers, PatchMerging, head) at --model-batch."""
import argparse
import json
import os
import statistics
import sys
from contextlib import contextmanager

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = ("EfficientViT_M0", "EfficientViT_M4", "EfficientViT_M5")


@contextmanager
def composed(on):
    old = os.environ.get("CREAM_IRPE_FUSED")
    if on:
        os.environ["CREAM_IRPE_FUSED"] = "0"
    try:
        yield
    finally:
        if on:
            if old is None:
                del os.environ["CREAM_IRPE_FUSED"]
            else:
                os.environ["CREAM_IRPE_FUSED"] = old


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
    """steps {name: fn} -> {name_ms, name_mean_ms, name_spread}: two rounds over the paths, so that drift hits all of them."""
    half = max(reps // 2, 2)
    runs, out = {k: [] for k in steps}, {}
    for _ in range(2):
        for name, fn in steps.items():
            runs[name] += timed(fn, half, warmup)
    for name in steps:
        q = statistics.quantiles(runs[name], n=4)
        med = statistics.median(runs[name])
        out[name + "_ms"], out[name + "_mean_ms"] = round(med, 4), round(statistics.fmean(runs[name]), 4)
        out[name + "_spread"] = round(0.5 * (q[2] - q[0]) / med, 4)
    return out


def stages(name):
    from cream_amd import efficientvit
    cfg = efficientvit.CONFIGS[name]
    res = cfg["img_size"] // cfg["patch_size"]
    out = []
    for i, (ed, nh, wd) in enumerate(zip(cfg["embed_dim"], cfg["num_heads"], cfg["window_size"])):
        out.append(dict(name=f"{name[-2:]}_stage{i + 1}", C=ed, heads=nh, res=res, window=wd, kernels=cfg["kernels"]))
        res = (res - 1) // 2 + 1
    return out


def layer(case, B, reps, warmup):
    from cream_amd import efficientvit, timing
    torch.manual_seed(0)
    C, res, nh = case["C"], case["res"], case["heads"]
    m = efficientvit.LocalWindowAttention(C, 16, nh, attn_ratio=C / (16 * nh), resolution=res, window_resolution=case["window"],
                                          kernels=case["kernels"])
    with torch.no_grad():
        m.attn.attention_biases.normal_(std=0.3)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.normal_(1.0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
    efficientvit.replace_batchnorm(m)
    m = m.cuda().eval()
    x = torch.randn(B, C, res, res, device="cuda").bfloat16()

    def step(off):
        def f():
            with composed(off), torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                m(x)
        return f

    r = interleaved({"fused": step(False), "composed": step(True)}, reps, warmup)
    r["ratio"] = round(r["composed_ms"] / r["fused_ms"], 3)
    timing.reset()
    timing.enable(True, only=("cga_attn_fwd",))
    for _ in range(5):
        step(False)()
    timing.enable(False)
    s = timing.summary().get("cga_attn_fwd")
    if s:
        r["cga_attn_fwd_ms"] = round(s["avg_ms"], 4)
        r["cga_attn_fwd_tflops"] = round(s["flops"] / (s["total_ms"] * 1e-3) / 1e12, 2)
    else:
        r["cga_attn_fwd_ms"] = None                   # the shape is not on the fused path
    return dict(case, part="attention_layer", B=B, **r)


COPY_RATE = 6.29e12          # bytes/s of a large device-to-device copy, the yardstick of profiles/NOTES_efficientvit.md


def _randomise_batchnorm(m):
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.normal_(1.0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)


def pair(case, B, reps, warmup):
    """The depthwise 3 x 3 + FFN pair of a stage shape: ONE launch on the token tensor (cream_amd/evit_ffn.py) against the two
    `Residual`s on the contiguous NCHW bf16 tensor the parent's path hands them."""
    from cream_amd import efficientvit, evit_ffn, timing
    torch.manual_seed(0)
    C, res = case["C"], case["res"]
    m = efficientvit._dw_ffn(C, res)
    _randomise_batchnorm(m)
    efficientvit.replace_batchnorm(m)
    m = m.cuda().eval()
    x = torch.randn(B, C, res, res, device="cuda").bfloat16()
    t = x.permute(0, 2, 3, 1).contiguous()
    routed = evit_ffn.usable_dwffn(torch.bfloat16, t.device, C, 2 * C, res, res)

    def fused():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            efficientvit.dw_ffn_tokens(m[0], m[1], t)

    def comp():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            m(x)

    r = interleaved({"fused": fused, "composed": comp}, reps, warmup)
    r["ratio"] = round(r["composed_ms"] / r["fused_ms"], 3)
    nbytes = 2 * B * res * res * C * 2 + 2 * (2 * C * C) * 2 + (9 + 1 + 2 + 1) * C * 4      # x in, y out, the weights once
    r["bytes"] = nbytes
    r["copy_rate_fraction"] = round(nbytes / (r["fused_ms"] * 1e-3) / COPY_RATE, 3)
    timing.reset()
    timing.enable(True, only=("evit_dwffn_fwd",))
    for _ in range(5):
        fused()
    timing.enable(False)
    s = timing.summary().get("evit_dwffn_fwd")
    r["evit_dwffn_fwd_ms"] = round(s["avg_ms"], 4) if s else None
    if s:
        r["evit_dwffn_fwd_tflops"] = round(s["flops"] / (s["total_ms"] * 1e-3) / 1e12, 2)
    return dict(name=case["name"], C=C, res=res, part="dw_ffn_pair", B=B, routed=routed, **r)


def _model(name, **kw):
    from cream_amd import efficientvit
    torch.manual_seed(0)
    return getattr(efficientvit, name)(num_classes=1000, fuse=True, **kw).cuda().eval()


def model_rates(name, B, reps, warmup):
    """tokens: the default path; parent: `fused_blocks=False`, the path before the token route (fused attention only);
    composed: CREAM_IRPE_FUSED=0."""
    model = _model(name)
    x = torch.randn(B, 3, 224, 224, device="cuda")

    def ev(off, blocks):
        def f():
            model.fused_blocks = blocks
            with composed(off), torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                model(x)
        return f

    r = interleaved({"tokens": ev(False, True), "parent": ev(False, False), "composed": ev(True, True)}, reps, warmup)
    out = dict(model=name, B=B)
    for k in ("tokens", "parent", "composed"):
        out[f"eval_{k}_img_s"] = round(B / r[k + "_mean_ms"] * 1e3, 1)        # speed_test.py: batch over the MEAN time
        out[f"eval_{k}_spread"] = r[k + "_spread"]
    out["eval_tokens_over_parent"] = round(out["eval_tokens_img_s"] / out["eval_parent_img_s"], 3)
    out["eval_tokens_over_composed"] = round(out["eval_tokens_img_s"] / out["eval_composed_img_s"], 3)
    return out


def model_split(name, B, reps, warmup):
    """Where the parent's path (`fused_blocks=False`) spends a forward pass: events between the parts of one pass, no
    synchronisation inside it, medians over the passes."""
    from cream_amd import efficientvit
    model = _model(name, fused_blocks=False)
    x = torch.randn(B, 3, 224, 224, device="cuda")
    parts = ("stem", "dw_ffn_pairs", "mixers", "patch_merging", "head")

    def one_pass():
        marks = []

        def mark(part):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((part, e))
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            mark(None)
            y = model.patch_embed(x)
            mark("stem")
            for stage in (model.blocks1, model.blocks2, model.blocks3):
                for m in stage:
                    if isinstance(m, efficientvit.EfficientViTBlock):
                        y = m.ffn0(m.dw0(y))
                        mark("dw_ffn_pairs")
                        y = m.mixer(y)
                        mark("mixers")
                        y = m.ffn1(m.dw1(y))
                        mark("dw_ffn_pairs")
                    elif isinstance(m, efficientvit.PatchMerging):
                        y = m(y)
                        mark("patch_merging")
                    else:
                        y = m(y)
                        mark("dw_ffn_pairs")
            model.head(torch.nn.functional.adaptive_avg_pool2d(y, 1).flatten(1))
            mark("head")
        torch.cuda.synchronize()
        ms = dict.fromkeys(parts, 0.0)
        for (_, a), (part, b) in zip(marks, marks[1:]):
            ms[part] += a.elapsed_time(b)
        return ms

    for _ in range(warmup):
        one_pass()
    runs = [one_pass() for _ in range(reps)]
    med = {p: statistics.median(r[p] for r in runs) for p in parts}
    total = sum(med.values())
    out = dict(model=name, B=B, part="parent_split", total_ms=round(total, 3))
    for p in parts:
        out[p + "_ms"], out[p + "_share"] = round(med[p], 3), round(med[p] / total, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--model-batch", type=int, default=2048)
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--pairs", action="store_true", help="the dw + FFN pair of every stage shape at --batch and --model-batch")
    ap.add_argument("--split", action="store_true", help="the parent path's time per part of the model at --model-batch")
    ap.add_argument("--skip-layers", action="store_true", help="leave the attention-layer leg out")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about speed"

    def emit(r):
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    if not a.skip_layers:
        for name in MODELS:
            for c in stages(name):
                emit(layer(c, a.batch, a.reps, a.warmup))
    if a.pairs:
        for name in MODELS:
            for c in stages(name):
                for B in (a.batch, a.model_batch):
                    emit(pair(c, B, a.reps, a.warmup))
    if a.split:
        for name in MODELS:
            emit(model_split(name, a.model_batch, max(a.reps // 3, 6), 3))
    if a.models:
        for name in MODELS:
            emit(model_rates(name, a.model_batch, max(a.reps // 3, 6), 3))


if __name__ == "__main__":
    main()
