#!/usr/bin/env python
"""A Mini-Swin block's attention half at window 12 (norm1, qkv, window attention, proj), forward + backward under bf16
autocast: the fused kernels (cream_amd/window_attn_mix_large.py with head transforms, cream_amd/window_attn_large.py without)
against the block's composed branch, same process, same data, runs interleaved.

    python tools/bench_window_attention_mix_large.py [--reps 20] [--warmup 3] [--batch 16] [--train] [--train-batch 0] [--out FILE]

The cases are the four stages of swin_base_patch4_window7_224to384_minivit_sharenum2 (image 384, window 12, heads 4 / 8 / 16 /
32 on maps of 96 / 48 / 24 / 12), each with head transforms (the student) and without (the plain Swin-B window12_384 teacher);
32 mixed heads are not covered by the kernels and are reported as such.  The tool puts the shapes it measures into the accepted
sets itself, so what it measures does not depend on what they hold.  Per case it prints one JSON line: median ms of each path,
the run-to-run spread (half the inter-quartile range of the repeated runs, as a fraction of the median), the ratio composed /
fused, `accept` (the fused median beats the composed one by more than the sum of the two spreads: the rule of
window_attn_mix_large.ACCEPTED), the peak of torch.cuda.max_memory_allocated above the bytes held before the run, and the
average of the kernels' own timing regions.  The composed path is the block's own fallback (CREAM_IRPE_FUSED=0 around the
call).  --train adds mini_swin('base', img_size=384, window_size=12) training steps (forward + backward, bf16 autocast),
images/s on each path with every covered recipe shape routed, at the largest batch of 8, 16, 32, 64 at which the composed step
fits in memory (--train-batch 0, the default; the line records the batch and whether the cap of 64 was reached)."""
import argparse
import json
import os
import statistics
import sys
from contextlib import contextmanager

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = [dict(name="stage1", H=4, res=96), dict(name="stage2", H=8, res=48), dict(name="stage3", H=16, res=24),
          dict(name="stage4", H=32, res=12)]
W = 12


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


def accept_all():
    from cream_amd import window_attn_mix_large as M
    shapes = frozenset((W, s["res"], s["res"], s["H"]) for s in STAGES)
    M.ACCEPTED, M.PLAIN_ACCEPTED, M.EXCLUDED, M.PLAIN_EXCLUDED = shapes, shapes, frozenset(), frozenset()


def interleaved(step, reps, warmup):
    """fused, composed, fused, composed halves, so that drift hits both -> dict of medians, spreads, peaks, ratio, accept"""
    half = max(reps // 2, 2)
    runs, peak, out = {"fused": [], "composed": []}, {}, {}
    for _ in range(2):
        for name, off in (("fused", False), ("composed", True)):
            ms, pk = timed(step(off), half, warmup)
            runs[name] += ms
            peak[name] = max(peak.get(name, 0), pk)
    for name in runs:
        med, spread = summary(runs[name])
        out[name + "_ms"] = round(med, 4)
        out[name + "_spread"] = round(spread, 4)
        out[name + "_peak_mb"] = round(peak[name] / 2 ** 20, 1)
    out["ratio"] = round(out["composed_ms"] / out["fused_ms"], 3)
    margin = out["fused_spread"] * out["fused_ms"] + out["composed_spread"] * out["composed_ms"]
    out["accept"] = bool(out["composed_ms"] - out["fused_ms"] > margin)
    return out


def layer(stage, mix, B, reps, warmup):
    from cream_amd import miniswin, timing
    H, res = stage["H"], stage["res"]
    case = dict(name=stage["name"] + ("_mixed" if mix else "_plain"), shape=[W, res, res, H], B=B)
    torch.manual_seed(0)
    blk = miniswin.SwinTransformerBlock(H * 32, (res, res), H, window_size=W, shift_size=W // 2, drop_path=[0.],
                                        is_transform_heads=mix)
    with torch.no_grad():
        blk.attn.relative_position_bias_table.normal_(std=0.3)
    blk.mlp, blk.norm2 = torch.nn.Identity(), torch.nn.Identity()          # the attention half alone
    blk = blk.cuda()
    shifted = blk.shift_size > 0
    x = torch.randn(B, res * res, H * 32, device="cuda", requires_grad=True)
    gy = torch.randn(B, res * res, H * 32, device="cuda")
    regions = ("window_attn_mix_large_fwd", "window_attn_mix_large_bwd") if mix else ("window_attn_large_fwd", "window_attn_large_bwd")

    def step(off):
        def f():
            with composed(off), torch.autocast("cuda", dtype=torch.bfloat16):
                y = blk.forward_feature(x, is_shift=shifted, layer_index=0)
            y.backward(gy)
            blk.zero_grad(set_to_none=True)
            x.grad = None
        return f

    timing.reset()
    timing.enable(True, only=regions)
    step(False)()
    timing.enable(False)
    if regions[0] not in timing.summary():
        return dict(case, covered=False)                                   # 32 mixed heads: composed whatever the sets hold
    res_ = interleaved(step, reps, warmup)
    # the kernels alone: the regions' events around the launches, after the layer timing so that they do not perturb it
    timing.reset()
    timing.enable(True, only=regions)
    for _ in range(5):
        step(False)()
    timing.enable(False)
    s = timing.summary()
    for name in regions:
        if name in s:
            res_[name + "_ms"] = round(s[name]["avg_ms"], 4)
            res_[name + "_tflops"] = round(s[name]["flops"] / s[name]["total_ms"] / 1e9, 2)
    return dict(case, covered=True, **res_)


def training(B, reps, warmup, cap=64):
    """B = 0: the largest batch of 8, 16, 32, ... (at most `cap`) at which a composed training step fits in memory."""
    from cream_amd import miniswin
    torch.manual_seed(0)
    model = miniswin.mini_swin('base', img_size=384, window_size=W).cuda().train()
    data = {}

    def step(off):
        def f():
            x, y = data["x"], data["y"]
            with composed(off), torch.autocast("cuda", dtype=torch.bfloat16):
                loss = torch.nn.functional.cross_entropy(model(x).float(), y)
            loss.backward()
            model.zero_grad(set_to_none=True)
        return f

    def set_batch(n):
        data["x"] = torch.randn(n, 3, 384, 384, device="cuda")
        data["y"] = torch.randint(0, 1000, (n,), device="cuda")

    searched = B == 0
    if searched:
        B, n = 0, 8
        while n <= cap:
            try:
                set_batch(n)
                step(True)()
                torch.cuda.synchronize()
                B = n
            except torch.cuda.OutOfMemoryError:
                model.zero_grad(set_to_none=True)
                break
            n *= 2
        data.clear()
        torch.cuda.empty_cache()
        assert B > 0, "the composed step does not fit at batch 8"
    set_batch(B)
    out = interleaved(step, reps, warmup)
    out["fused_img_s"] = round(B / out["fused_ms"] * 1e3, 1)
    out["composed_img_s"] = round(B / out["composed_ms"] * 1e3, 1)
    return dict(model="mini_swin_base_384_w12_train", B=B, batch_searched=searched, batch_cap=cap, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-batch", type=int, default=0, help="0: the largest of 8, 16, 32, 64 the composed path fits")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    accept_all()

    def emit(r):
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    for stage in STAGES:
        for mix in (True, False):
            emit(layer(stage, mix, a.batch, a.reps, a.warmup))
    if a.train:
        emit(training(a.train_batch, max(a.reps // 2, 6), 2))


if __name__ == "__main__":
    main()
