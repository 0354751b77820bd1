#!/usr/bin/env python
"""One `MiniAttention` layer with head transforms, forward + backward under bf16 autocast: the fused kernels
(cream_amd/mini_attn.py) against the module's composed branch, same process, same data, runs interleaved.

    python tools/bench_mini_attention.py [--reps 30] [--warmup 5] [--step]

Per shape it prints one JSON line: median ms of each path, the run-to-run spread (half the inter-quartile range of the
repeated runs, as a fraction of the median), the ratio composed / fused, and the peak of torch.cuda.max_memory_allocated
above the bytes held before the run.  The composed path is selected through the module's own fallback (CREAM_IRPE_FUSED=0
around the call).  --step adds a mini_deit('small') train step (B = 64, AdamW), images/s on each path."""
import argparse
import json
import os
import statistics
import sys
from contextlib import contextmanager

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [dict(H=3, B=128, L=196), dict(H=6, B=128, L=196), dict(H=12, B=64, L=196), dict(H=12, B=32, L=576),
          # small batches (inference): few workgroups per launch, where the launch count of the fused backward weighs most
          dict(H=3, B=1, L=196), dict(H=12, B=1, L=196), dict(H=12, B=1, L=576)]


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


def layer(shape, reps, warmup):
    from cream_amd import minivit, timing
    from cream_amd.irpe import get_rpe_config
    H, B, L = shape["H"], shape["B"], shape["L"]
    cfg = get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=True, skip=0, rpe_on='k')
    torch.manual_seed(0)
    m = minivit.MiniAttention(H * 64, num_heads=H, qkv_bias=True, rpe_config=cfg, repeated_times=1, use_transform=True).cuda()
    with torch.no_grad():
        m.rpe_k.instances[0].lookup_table_weight.normal_(std=0.3)
        for c in (m.conv_l.instances[0], m.conv_w.instances[0]):
            c.weight.copy_((torch.eye(H) + 0.3 * torch.randn(H, H)).reshape(H, H, 1, 1))
    x = torch.randn(B, L, H * 64, device="cuda", requires_grad=True)
    gy = torch.randn(B, L, H * 64, device="cuda")

    def step(off):
        def f():
            with composed(off), torch.autocast("cuda", dtype=torch.bfloat16):
                y = m(x)
            y.backward(gy)
            m.zero_grad(set_to_none=True)
            x.grad = None
        return f

    timing.reset(); timing.enable(True)
    step(False)()
    timing.enable(False)
    took_fused = "mini_attn_fwd" in timing.summary()
    res = {}
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
        res[name + "_ms"] = round(med, 4)
        res[name + "_spread"] = round(spread, 4)
        res[name + "_peak_mb"] = round(peak[name] / 2 ** 20, 1)
    res["ratio"] = round(res["composed_ms"] / res["fused_ms"], 3)
    res["fused_path_taken"] = took_fused
    return dict(shape, E=H * 64, **res)


def train_step(reps, warmup, B=64):
    from cream_amd import minivit
    torch.manual_seed(0)
    model = minivit.mini_deit('small').cuda().train()
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
    return dict(model="mini_deit_small", B=B, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = [layer(s, a.reps, a.warmup) for s in SHAPES]
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
