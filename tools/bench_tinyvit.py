#!/usr/bin/env python
"""TinyViT blocks at the three stage shapes of tiny_vit_21m_224, forward + backward at B = 128 under bf16 autocast: the fused
routings (cream_amd/tinyvit.py: window attention, token-layout depthwise convolution) against the composed branches of the same
code, same process, same data, runs interleaved.

    python tools/bench_tinyvit.py [--reps 30] [--warmup 5] [--models] [--out FILE]

Per stage shape it prints one JSON line for the attention half, one for the local-convolution half (with BatchNorm on the
(B L, C) view, the (B L, C, 1, 1) view, and the eval-mode fold) and one for the whole block: median ms of each path, the
run-to-run spread (half the inter-quartile range as a fraction of the median), the ratio composed / fused, peak memory above
the bytes held before the run, and for the convolution kernels the achieved bytes/s (bytes counted from shapes) against the
HBM peak (8.0 TB/s by the data sheet, 6.29 TB/s as a float4 copy measures it).  Composed means CREAM_IRPE_FUSED=0 and
fused_local_conv=False.  --models adds evaluation and training-step (forward + backward) images/s of tiny_vit_5m_224 and
tiny_vit_21m_224."""
import argparse
import json
import os
import statistics
import sys
from contextlib import contextmanager

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
STAGES = [dict(name="21m_stage1", C=192, H=6, res=28, window=7), dict(name="21m_stage2", C=384, H=12, res=14, window=14),
          dict(name="21m_stage3", C=576, H=18, res=7, window=7)]


@contextmanager
def composed(on, blocks):
    old_env, old = os.environ.get("CREAM_IRPE_FUSED"), [b.fused_local_conv for b in blocks]
    if on:
        os.environ["CREAM_IRPE_FUSED"] = "0"
        for b in blocks:
            b.fused_local_conv = False
    try:
        yield
    finally:
        if on:
            for b, f in zip(blocks, old):
                b.fused_local_conv = f
            if old_env is None:
                del os.environ["CREAM_IRPE_FUSED"]
            else:
                os.environ["CREAM_IRPE_FUSED"] = old_env


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


def stage(case, B, reps, warmup):
    from cream_amd import timing, tinyvit, token_conv
    torch.manual_seed(0)
    C, res = case["C"], case["res"]
    blk = tinyvit.TinyViTBlock(C, (res, res), case["H"], window_size=case["window"])
    with torch.no_grad():
        blk.attn.attention_biases.normal_(std=0.3)
    blk = blk.cuda().train()
    x = torch.randn(B, res * res, C, device="cuda", requires_grad=True)
    xb = x.detach().bfloat16().requires_grad_(True)           # the stream is bf16 after a block's convolution
    gy = torch.randn(B, res * res, C, device="cuda")

    def conv_nc11(t):
        """The fused convolution with the block's BatchNorm module on the (B L, C, 1, 1) view — the alternative to the
        (B L, C) view the block uses."""
        c, bn = blk.local_conv.c, blk.local_conv.bn
        z = token_conv.token_dwconv3(t, c.weight, None, (res, res))
        return bn(z.view(-1, C, 1, 1)).view(t.shape)

    def step(fn, inp, off, train=True):
        def f():
            blk.local_conv.train(train)                       # BatchNorm's mode: batch statistics, or the eval-mode fold
            with composed(off, [blk]), torch.autocast("cuda", dtype=torch.bfloat16):
                y = fn(inp)
            y.backward(gy.to(y.dtype))
            blk.zero_grad(set_to_none=True)
            inp.grad = None
        return f

    lines = []
    r = interleaved({"fused": step(lambda t: t + blk.window_attention(t), x, False),
                     "composed": step(lambda t: t + blk.window_attention(t), x, True)}, reps, warmup)
    r["ratio"] = round(r["composed_ms"] / r["fused_ms"], 3)
    lines.append(dict(case, part="attention", B=B, **r))
    r = interleaved({"fused": step(blk.local_convolution, xb, False), "fused_nc11": step(conv_nc11, xb, False),
                     "composed": step(blk.local_convolution, xb, True), "fused_eval": step(blk.local_convolution, xb, False, train=False),
                     "composed_eval": step(blk.local_convolution, xb, True, train=False)}, reps, warmup)
    r["ratio"] = round(r["composed_ms"] / r["fused_ms"], 3)
    r["ratio_nc11"] = round(r["composed_ms"] / r["fused_nc11_ms"], 3)
    r["ratio_eval"] = round(r["composed_eval_ms"] / r["fused_eval_ms"], 3)
    # the kernels alone: the regions' events around the launches
    timing.reset()
    timing.enable(True, only=("token_dwconv3_fwd", "token_dwconv3_bwd"))
    for _ in range(5):
        step(blk.local_convolution, xb, False)()
    timing.enable(False)
    s = timing.summary()
    for name in ("token_dwconv3_fwd", "token_dwconv3_bwd"):
        if name in s:
            rate = s[name]["bytes"] / (s[name]["total_ms"] * 1e-3)
            r[name + "_ms"] = round(s[name]["avg_ms"], 4)
            r[name + "_tb_s"] = round(rate / 1e12, 3)
            r[name + "_of_hbm_spec"] = round(rate / HBM_SPEC, 3)
            r[name + "_of_hbm_copy"] = round(rate / HBM_COPY, 3)
    lines.append(dict(case, part="local_conv", B=B, **r))
    r = interleaved({"fused": step(blk, x, False), "composed": step(blk, x, True)}, reps, warmup)
    r["ratio"] = round(r["composed_ms"] / r["fused_ms"], 3)
    lines.append(dict(case, part="block", B=B, **r))
    return lines


def model_rates(name, B, reps, warmup):
    from cream_amd import tinyvit
    torch.manual_seed(0)
    model = getattr(tinyvit, name)().cuda()
    blocks = [b for layer in model.layers[1:] for b in layer.blocks]
    x = torch.randn(B, 3, 224, 224, device="cuda")
    out = dict(model=name, B=B)

    def ev(off):
        def f():
            with composed(off, blocks), torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                model(x)
        return f

    def tr(off):
        def f():
            with composed(off, blocks), torch.autocast("cuda", dtype=torch.bfloat16):
                y = model(x)
            y.float().sum().backward()
            model.zero_grad(set_to_none=True)
        return f

    for mode, mk in (("eval", ev), ("train", tr)):
        model.train(mode == "train")
        r = interleaved({"fused": mk(False), "composed": mk(True)}, reps, warmup)
        for k in ("fused", "composed"):
            out[f"{mode}_{k}_img_s"] = round(B / r[k + "_ms"] * 1e3, 1)
            out[f"{mode}_{k}_spread"] = r[k + "_spread"]
            out[f"{mode}_{k}_peak_mb"] = r[k + "_peak_mb"]
        out[f"{mode}_ratio"] = round(out[f"{mode}_fused_img_s"] / out[f"{mode}_composed_img_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about speed"

    def emit(r):
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    for c in STAGES:
        for r in stage(c, a.batch, a.reps, a.warmup):
            emit(r)
    if a.models:
        for name in ("tiny_vit_5m_224", "tiny_vit_21m_224"):
            emit(model_rates(name, a.batch, max(a.reps // 3, 6), 3))


if __name__ == "__main__":
    main()
