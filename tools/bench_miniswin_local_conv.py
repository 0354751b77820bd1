#!/usr/bin/env python
"""Mini-Swin's local convolution (LayerNorm, then x + depthwise 7 x 7 convolution; cream_amd/miniswin.py
`SwinTransformerBlock.local_convolution`) at the stage shapes of the published recipes, forward + backward under bf16 autocast:
the fused routing (cream_amd.token_conv.token_dwconv7 on csrc/token_dwconv7.hip) against the composed lines of the same code
(`fused_local_conv=False`: the transposes to NCHW and back around the framework's convolution), same process, same data, runs
interleaved.

    python tools/bench_miniswin_local_conv.py [--reps 30] [--warmup 5] [--step] [--out FILE]

Per shape it prints one JSON line: median ms of each path, the run-to-run spread (half the inter-quartile range as a fraction of
the median), the ratio composed / fused, peak memory above the bytes held before the run, and for the two kernel regions the
time of the launches alone with the achieved bytes/s (bytes counted from shapes) against the HBM peak (8.0 TB/s by the data
sheet, 6.29 TB/s as a float4 copy measures it).  --step adds the `mini_swin('tiny')` training step (B = 64, AdamW, bf16
autocast) with `fused_local_conv` on and off."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
SHAPES = [dict(name="T_stage1", res=56, C=96, B=128), dict(name="T_stage2", res=28, C=192, B=128),
          dict(name="T_stage3", res=14, C=384, B=128), dict(name="T_stage4", res=7, C=768, B=128),
          dict(name="B_stage1", res=56, C=128, B=128), dict(name="B384_stage1", res=96, C=128, B=16),
          dict(name="B384_stage4", res=12, C=1024, B=16)]
REGIONS = ("token_dwconv7_fwd", "token_dwconv7_bwd")


def timed(fn, reps, warmup):
    """-> (list of ms per run, peak bytes above the starting allocation)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms, torch.cuda.max_memory_allocated() - base


def summary(ms):
    q = statistics.quantiles(ms, n=4)
    med = statistics.median(ms)
    return med, 0.5 * (q[2] - q[0]) / med


def interleaved(steps, reps, warmup):
    """steps {name: fn} -> {name_ms, name_spread, name_peak_mb}: two rounds over the paths, so that drift hits all of them."""
    half = max(reps // 2, 2)
    runs, peak, out = {k: [] for k in steps}, {}, {}
    for _ in range(2):
        for name, fn in steps.items():
            ms, pk = timed(fn, half, warmup)
            runs[name] += ms
            peak[name] = max(peak.get(name, 0), pk)
    for name in steps:
        med, spread = summary(runs[name])
        out[name + "_ms"], out[name + "_spread"], out[name + "_peak_mb"] = round(med, 4), round(spread, 4), round(peak[name] / 2 ** 20, 1)
    return out


def layer(case, reps, warmup):
    from cream_amd import miniswin, timing
    torch.manual_seed(0)
    C, res, B = case["C"], case["res"], case["B"]
    blk = miniswin.SwinTransformerBlock(dim=C, input_resolution=(res, res), num_heads=C // 32, window_size=7 if res % 7 == 0 else 12,
                                        shift_size=0, drop_path=(0.,), is_sep_layernorm=True, is_transform_FFN=True,
                                        is_transform_heads=True).cuda().train()
    x = torch.randn(B, res * res, C, device="cuda", requires_grad=True)
    gy = torch.randn(B, res * res, C, device="cuda")

    def step(fused):
        def f():
            blk.fused_local_conv = fused
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = blk.local_convolution(x, 0)
            y.backward(gy)
            blk.zero_grad(set_to_none=True)
            x.grad = None
        return f

    r = interleaved({"fused": step(True), "composed": step(False)}, reps, warmup)
    r["ratio"] = round(r["composed_ms"] / r["fused_ms"], 3)
    timing.reset()
    timing.enable(True, only=REGIONS)                       # the kernels alone: the regions' events around the launches
    for _ in range(5):
        step(True)()
    timing.enable(False)
    s = timing.summary()
    for name in REGIONS:
        rate = s[name]["bytes"] / (s[name]["total_ms"] * 1e-3)
        r[name + "_ms"] = round(s[name]["avg_ms"], 4)
        r[name + "_bytes"] = int(s[name]["bytes"] // s[name]["launches"])
        r[name + "_tb_s"] = round(rate / 1e12, 3)
        r[name + "_of_hbm_spec"] = round(rate / HBM_SPEC, 3)
        r[name + "_of_hbm_copy"] = round(rate / HBM_COPY, 3)
    return dict(case, part="local_convolution", **r)


def train_step(B, reps, warmup):
    from cream_amd import miniswin
    torch.manual_seed(0)
    model = miniswin.mini_swin('tiny').cuda().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.05)
    x = torch.randn(B, 3, 224, 224, device="cuda")
    target = torch.randint(0, 1000, (B,), device="cuda")

    def step(fused):
        def f():
            model.fused_local_conv = fused
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = torch.nn.functional.cross_entropy(model(x).float(), target)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return f

    r = interleaved({"fused": step(True), "composed": step(False)}, reps, warmup)
    out = dict(model="mini_swin_tiny", part="train_step", B=B, **r)
    for k in ("fused", "composed"):
        out[k + "_img_s"] = round(B / r[k + "_ms"] * 1e3, 1)
    out["ratio"] = round(r["composed_ms"] / r["fused_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about speed"

    def emit(r):
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    for c in SHAPES:
        emit(layer(c, a.reps, a.warmup))
    if a.step:
        emit(train_step(64, max(a.reps // 2, 8), 3))


if __name__ == "__main__":
    main()
