#!/usr/bin/env python
"""One S3 block's attention half (norm1, qkv, 14 x 14 window attention, proj), forward + backward under bf16 autocast: the
fused kernels (cream_amd/window_attn_large.py) against the block's composed branch, same process, same data, runs interleaved.

    python tools/bench_window_attention_large.py [--reps 30] [--warmup 5] [--eval] [--out FILE]

Per layer case it prints one JSON line: median ms of each path, the run-to-run spread (half the inter-quartile range of the
repeated runs, as a fraction of the median), the ratio composed / fused, the peak of torch.cuda.max_memory_allocated above the
bytes held before the run, and the average of the kernels' own timing regions (window_attn_large_fwd / _bwd).  The composed
path is selected through the block's own fallback (CREAM_IRPE_FUSED=0 around the call).  --eval adds s3('T') and s3('S')
evaluation (B = 64, eval mode, no grad), images/s on each path."""
import argparse
import json
import os
import statistics
import sys
from contextlib import contextmanager

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [dict(name="s3_stage3", H=12, res=14, B=128, shift=0),           # one window per image, 12 heads
         dict(name="s3s_stage1", H=3, res=56, B=128, shift=7)]           # 16 windows per image, shifted and masked


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
    from cream_amd import s3, timing
    H, res, B = case["H"], case["res"], case["B"]
    torch.manual_seed(0)
    blk = s3.SwinTransformerBlock(H * 32, (res, res), H, window_size=14, shift_size=case["shift"])
    with torch.no_grad():
        blk.attn.relative_position_bias_table.normal_(std=0.3)
    blk.mlp, blk.norm2 = torch.nn.Identity(), torch.nn.Identity()          # the attention half alone
    blk = blk.cuda()
    x = torch.randn(B, res * res, H * 32, device="cuda", requires_grad=True)
    gy = torch.randn(B, res * res, H * 32, device="cuda")

    def step(off):
        def f():
            with composed(off), torch.autocast("cuda", dtype=torch.bfloat16):
                y = blk(x)
            y.backward(gy)
            blk.zero_grad(set_to_none=True)
            x.grad = None
        return f

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
    # the kernels alone: the regions' events around the launches, after the layer timing so that they do not perturb it
    timing.reset()
    timing.enable(True, only=("window_attn_large_fwd", "window_attn_large_bwd"))
    for _ in range(5):
        step(False)()
    timing.enable(False)
    s = timing.summary()
    res_["fused_path_taken"] = "window_attn_large_fwd" in s
    for name in ("window_attn_large_fwd", "window_attn_large_bwd"):
        if name in s:
            res_[name + "_ms"] = round(s[name]["avg_ms"], 4)
            res_[name + "_tflops"] = round(s[name]["flops"] / s[name]["total_ms"] / 1e9, 2)
    return dict(case, E=H * 32, **res_)


def evaluation(size, reps, warmup, B=64):
    from cream_amd import s3
    torch.manual_seed(0)
    model = s3.s3(size).cuda().eval()
    x = torch.randn(B, 3, 224, 224, device="cuda")
    out = {}

    def step(off):
        def f():
            with composed(off), torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                model(x)
        return f

    for name, off in (("fused", False), ("composed", True)):
        ms, pk = timed(step(off), reps, warmup)
        med, spread = summary(ms)
        out[name + "_img_s"] = round(B / med * 1e3, 1)
        out[name + "_spread"] = round(spread, 4)
        out[name + "_peak_mb"] = round(pk / 2 ** 20, 1)
    out["ratio"] = round(out["fused_img_s"] / out["composed_img_s"], 3)
    return dict(model=f"s3_{size}_eval", B=B, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = [layer(c, a.reps, a.warmup) for c in CASES]
    if a.eval:
        lines += [evaluation(size, max(a.reps // 3, 5), 3) for size in ("T", "S")]
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
