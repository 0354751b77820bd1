#!/usr/bin/env python
"""One Mini-Swin block repeat's attention half (norm1, qkv, window attention, proj), forward + backward under bf16 autocast:
the fused kernels (cream_amd/window_attn.py) against the block's composed branch, same process, same data, runs interleaved.

    python tools/bench_window_attention.py [--reps 30] [--warmup 5] [--step] [--out FILE]

Per layer case it prints one JSON line: median ms of each path, the run-to-run spread (half the inter-quartile range of the
repeated runs, as a fraction of the median), the ratio composed / fused, and the peak of torch.cuda.max_memory_allocated
above the bytes held before the run.  The composed path is selected through the block's own fallback (CREAM_IRPE_FUSED=0
around the call).  --step adds a mini_swin('tiny') train step (B = 64, AdamW), images/s on each path."""
import argparse
import json
import os
import statistics
import sys
from contextlib import contextmanager

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [dict(name="tiny_stage1", H=3, res=56, B=128), dict(name="tiny_stage3", H=12, res=14, B=128),
         dict(name="base_stage3", H=16, res=14, B=128),
         # plain Swin (no head transforms) and a small batch, where the launch count weighs most
         dict(name="plain_stage1", H=3, res=56, B=128, mix=False), dict(name="tiny_stage1_b1", H=3, res=56, B=1)]


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


def layer(case, reps, warmup):
    from cream_amd import miniswin, timing
    H, res, B, mix = case["H"], case["res"], case["B"], case.get("mix", True)
    torch.manual_seed(0)
    blk = miniswin.SwinTransformerBlock(H * 32, (res, res), H, window_size=7, shift_size=3, drop_path=[0.], is_transform_heads=mix)
    with torch.no_grad():
        blk.attn.relative_position_bias_table.normal_(std=0.3)
        if mix:
            for m in (blk.proj_l[0], blk.proj_w[0]):
                m.weight.copy_(torch.eye(H) + 0.3 * torch.randn(H, H))
    blk.mlp, blk.norm2 = torch.nn.Identity(), torch.nn.Identity()          # the attention half alone
    blk = blk.cuda()
    x = torch.randn(B, res * res, H * 32, device="cuda", requires_grad=True)
    gy = torch.randn(B, res * res, H * 32, device="cuda")

    def step(off):
        def f():
            with composed(off), torch.autocast("cuda", dtype=torch.bfloat16):
                y = blk.forward_feature(x, is_shift=True, layer_index=0)
            y.backward(gy)
            blk.zero_grad(set_to_none=True)
            x.grad = None
        return f

    timing.reset()
    timing.enable(True)
    step(False)()
    timing.enable(False)
    took_fused = "window_attn_fwd" in timing.summary()
    res_ = {}
    # interleaved: fused, composed, fused, composed halves, so that drift hits both
    half = max(reps // 2, 2)
    runs = {"fused": [], "composed": []}
    peak = {}
    for _ in range(2):
        for name, off in (("fused", False), ("composed", True)):
            ms, pk = timed(step(off), half, warmup)
            runs[name] += ms
            peak[name] = max(peak.get(name, 0), pk)
    for name in runs:
        med, spread = summary(runs[name])
        res_[name + "_ms"] = round(med, 4)
        res_[name + "_spread"] = round(spread, 4)
        res_[name + "_peak_mb"] = round(peak[name] / 2 ** 20, 1)
    res_["ratio"] = round(res_["composed_ms"] / res_["fused_ms"], 3)
    res_["fused_path_taken"] = took_fused
    return dict(case, E=H * 32, **res_)


def train_step(reps, warmup, B=64):
    from cream_amd import miniswin
    torch.manual_seed(0)
    model = miniswin.mini_swin('tiny').cuda().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    x = torch.randn(B, 3, 224, 224, device="cuda")
    t = torch.randint(0, 1000, (B,), device="cuda")
    out = {}

    def step(off):
        def f():
            with composed(off), torch.autocast("cuda", dtype=torch.bfloat16):
                loss = torch.nn.functional.cross_entropy(model(x).float(), t)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return f

    for name, off in (("fused", False), ("composed", True)):
        ms, pk = timed(step(off), reps, warmup)
        med, spread = summary(ms)
        out[name + "_img_s"] = round(B / med * 1e3, 1)
        out[name + "_spread"] = round(spread, 4)
        out[name + "_peak_mb"] = round(pk / 2 ** 20, 1)
    return dict(model="mini_swin_tiny", B=B, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = [layer(c, a.reps, a.warmup) for c in CASES]
    if a.step:
        lines.append(train_step(max(a.reps // 3, 5), 3))
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
