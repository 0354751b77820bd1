#!/usr/bin/env python
"""One TinyViT block's attention half (norm, qkv, window attention with the offset bias, proj) at the windows of
tiny_vit_21m_384 / _512, forward + backward under bf16 autocast: the streaming kernels (cream_amd/window_attn_xl.py) against the
block's composed branch, same process, same data, runs interleaved.

    python tools/bench_window_attention_xl.py [--reps 30] [--warmup 5] [--batch 128] [--models] [--out FILE]

Per layer case it prints one JSON line: median ms of each path, the run-to-run spread (half the inter-quartile range of the
repeated runs, as a fraction of the median), the ratio composed / fused, `accepted` (the fused median beats the composed one by
more than the sum of the two spreads: the rule for routing a shape by default), the peak of torch.cuda.max_memory_allocated
above the bytes held before the run, and the average of the kernels' own timing regions (window_attn_xl_fwd / _bwd).  The
composed path is selected through the block's own fallback (CREAM_IRPE_FUSED=0 around the call).  --models adds
tiny_vit_21m_384 and tiny_vit_21m_512, evaluation (eval mode, no grad) and a training step (forward, backward, SGD), images/s on
each path."""
import argparse
import json
import os
import statistics
import sys
from contextlib import contextmanager

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the attention shapes of the two models
CASES = [dict(name="384_stage2", w=24, res=24, H=12),           # one 576-token window per image
         dict(name="512_stage1", w=16, res=64, H=6),            # 16 windows of 256 tokens per image
         dict(name="512_stage2", w=32, res=32, H=12),           # one 1024-token window per image
         dict(name="512_stage3", w=16, res=16, H=18),           # one 256-token window per image
         # the narrow shapes that the tests run: a shape is routed by default only once it has been measured here
         dict(name="narrow_w16_32x32_h6", w=16, res=32, H=6),
         dict(name="narrow_w16_32x32_h2", w=16, res=32, H=2),
         dict(name="narrow_w24_24x24_h3", w=24, res=24, H=3),
         dict(name="narrow_w16_16x16_h2", w=16, res=16, H=2)]
REGIONS = ("window_attn_xl_fwd", "window_attn_xl_bwd")


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


def interleaved(step, reps, warmup):
    """fused, composed, fused, composed halves, so that drift hits both -> {name: (median ms, spread, peak bytes)}"""
    half = max(reps // 2, 2)
    runs, peak = {"fused": [], "composed": []}, {}
    for _ in range(2):
        for name, off in (("fused", False), ("composed", True)):
            ms, pk = timed(step(off), half, warmup)
            runs[name] += ms
            peak[name] = max(peak.get(name, 0), pk)
            torch.cuda.empty_cache()
    return {name: summary(runs[name]) + (peak[name],) for name in runs}


def layer(case, B, reps, warmup):
    from cream_amd import timing, tinyvit, window_attn_xl
    H, res, w = case["H"], case["res"], case["w"]
    window_attn_xl.ACCEPTED |= {(w, res, res, H)}          # measuring is what puts a shape on that list: route it for this run
    torch.manual_seed(0)
    blk = tinyvit.TinyViTBlock(H * 32, (res, res), H, window_size=w)
    with torch.no_grad():
        blk.attn.attention_biases.normal_(std=0.3)
    blk = blk.cuda()
    x = torch.randn(B, res * res, H * 32, device="cuda", requires_grad=True)
    gy = torch.randn(B, res * res, H * 32, device="cuda")

    def step(off):
        def f():
            with composed(off), torch.autocast("cuda", dtype=torch.bfloat16):
                y = blk.window_attention(x)              # the attention half alone
            y.backward(gy)
            blk.zero_grad(set_to_none=True)
            x.grad = None
        return f

    r = {}
    for name, (med, spread, pk) in interleaved(step, reps, warmup).items():
        r[name + "_ms"], r[name + "_spread"], r[name + "_peak_mb"] = round(med, 4), round(spread, 4), round(pk / 2 ** 20, 1)
    r["ratio"] = round(r["composed_ms"] / r["fused_ms"], 3)
    r["accepted"] = r["composed_ms"] - r["fused_ms"] > r["composed_ms"] * r["composed_spread"] + r["fused_ms"] * r["fused_spread"]
    # the kernels alone: the regions' events around the launches, after the layer timing so that they do not perturb it
    timing.reset()
    timing.enable(True, only=REGIONS)
    for _ in range(5):
        step(False)()
    timing.enable(False)
    s = timing.summary()
    r["fused_path_taken"] = REGIONS[0] in s
    for name in REGIONS:
        if name in s:
            r[name + "_ms"] = round(s[name]["avg_ms"], 4)
            r[name + "_tflops"] = round(s[name]["flops"] / s[name]["total_ms"] / 1e9, 2)
    return dict(case, B=B, E=H * 32, **r)


def whole_model(name, train, B, reps, warmup):
    from cream_amd import tinyvit
    torch.manual_seed(0)
    model = getattr(tinyvit, name)(num_classes=1000).cuda()
    model.train(train)
    size = int(name.rsplit("_", 1)[1])
    x = torch.randn(B, 3, size, size, device="cuda")
    opt = torch.optim.SGD(model.parameters(), lr=1e-3) if train else None

    def step(off):
        def f():
            if not train:
                with composed(off), torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    model(x)
                return
            with composed(off), torch.autocast("cuda", dtype=torch.bfloat16):
                loss = model(x).float().logsumexp(-1).mean()
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return f

    r = {}
    for path, (med, spread, pk) in interleaved(step, reps, warmup).items():
        r[path + "_img_s"], r[path + "_spread"], r[path + "_peak_mb"] = round(B / med * 1e3, 1), round(spread, 4), round(pk / 2 ** 20, 1)
    r["ratio"] = round(r["fused_img_s"] / r["composed_img_s"], 3)
    return dict(model=name, mode="train" if train else "eval", B=B, **r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--model-batch", type=int, default=32)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    def emit(r):
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    for c in CASES:
        emit(layer(c, a.batch, a.reps, a.warmup))
    if a.models:
        for name in ("tiny_vit_21m_384", "tiny_vit_21m_512"):
            for train in (False, True):
                emit(whole_model(name, train, a.model_batch, max(a.reps // 3, 10), 3))


if __name__ == "__main__":
    main()
