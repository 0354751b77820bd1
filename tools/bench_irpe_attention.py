"""BASELINE config 4: DeiT-base-384 + iRPE product / contextual (rpe_ops fwd/bwd), B = 64, H = 12,
L = 577, head_dim 64, 50 buckets — ONE RPEAttention layer forward + backward on the MI355X
(after the standalone rpe_index micro-benchmark, "full RPEAttention fwd/bwd for
rpe_on in {k, qkv}").  Reports ms per fwd+bwd, the share of the rpe_index kernels (HIP events on
the launch stream, cream_amd.timing) and their achieved HBM GB/s against the algorithmic bytes.

    python tools/bench_irpe_attention.py > gpurun_out/irpe_attention.jsonl

DETR leg (`--leg detr`; `--leg deit` is the above alone, default both): DETR-with-iRPE's encoder self-attention with the
published recipe — N = 2, 8 heads of 32, 81 buckets on k, a 25 x 34 map (an 800 x 1088 image at stride 32, L = 850) with
the right third of image 1 padded, dropout 0.1, bf16 autocast, forward + backward — on the fused kernels
(csrc/irpe_attn_x.hip) against the composed path (CREAM_IRPE_FUSED=0) in the same process: median of 30 steps timed one
by one with HIP events after 5 warm-up steps, and the peak of torch.cuda.max_memory_allocated over a step of each.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cream_amd import timing
from cream_amd.irpe import get_rpe_config
from cream_amd.rpe_attention import RPEAttention

dev = torch.device("cuda")
leg = sys.argv[sys.argv.index("--leg") + 1] if "--leg" in sys.argv else "all"
assert leg in ("all", "deit", "detr"), leg
B, L, C, H = 64, 577, 768, 12
for rpe_on in ("k", "qkv") if leg in ("all", "deit") else ():
    for dtype in (torch.bfloat16, torch.float32):
        torch.manual_seed(0)
        cfg = get_rpe_config(ratio=1.9, method="product", mode="ctx", shared_head=True, skip=1, rpe_on=rpe_on)
        m = RPEAttention(C, num_heads=H, qkv_bias=True, rpe_config=cfg).to(dev)
        x = torch.randn(B, L, C, device=dev, requires_grad=True)
        g = torch.randn(B, L, C, device=dev)

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
                y = m(x)
            y.backward(g)
            x.grad = None
            for p in m.parameters():
                p.grad = None

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        timing.reset()
        timing.enable(True, only=("rpe_index_fwd", "rpe_index_bwd", "irpe_attn_fwd", "irpe_attn_bwd"))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 10
        a.record()
        for _ in range(n):
            step()
        b.record()
        torch.cuda.synchronize()
        timing.enable(False)
        ks = timing.summary()
        rec = dict(workload=f"RPEAttention fwd+bwd, DeiT-B-384 iRPE product-ctx rpe_on={rpe_on}", B=B, H=H, L=L,
                   dtype=str(dtype).split(".")[-1], ms_per_fwd_bwd=round(a.elapsed_time(b) / n, 3),
                   kernels={k: dict(launches=v["launches"], avg_us=round(v["avg_ms"] * 1e3, 1),
                                    total_ms_per_iter=round(v["total_ms"] / n, 3),
                                    GBps=round(v["bytes"] / (v["total_ms"] * 1e-3) / 1e9, 1) if v["bytes"] else None,
                                    TFLOPs=round(v["flops"] / (v["total_ms"] * 1e-3) / 1e12, 1) if v.get("flops") else None)
                            for k, v in sorted(ks.items())})
        print(json.dumps(rec), flush=True)


def detr_leg(steps=30, warmup=5):
    from cream_amd.detr_attention import RPEMultiheadAttention
    N, E, heads, hw = 2, 256, 8, (25, 34)
    Ld = hw[0] * hw[1]
    torch.manual_seed(0)
    cfg = get_rpe_config(ratio=2.0, method="product", mode="ctx", shared_head=True, skip=0, rpe_on="k")
    att = RPEMultiheadAttention(E, heads, dropout=0.1, rpe_config=cfg).to(dev).train()
    src = torch.randn(Ld, N, E, device=dev, requires_grad=True)
    pos = torch.randn(Ld, N, E, device=dev)
    gy = torch.randn(Ld, N, E, device=dev)
    pad = torch.zeros(N, *hw, dtype=torch.bool)
    pad[1, :, hw[1] - hw[1] // 3:] = True
    pad = pad.flatten(1).to(dev)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            qk = src + pos
            y = att(qk, qk, src, key_padding_mask=pad, need_weights=False, hw=hw)[0]
        y.backward(gy.to(y.dtype))
        src.grad = None
        for p in att.parameters():
            p.grad = None

    res = {}
    for name, env in (("fused", "1"), ("composed", "0")):
        os.environ["CREAM_IRPE_FUSED"] = env
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        timing.reset()
        timing.enable(True, only=("rpe_index_fwd", "rpe_index_bwd", "irpe_attn_fwd", "irpe_attn_bwd"))
        step()
        timing.enable(False)
        regions = sorted(timing.summary())
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        res[name] = dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), regions=regions,
                         peak_MB_over_resident=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2))
    os.environ.pop("CREAM_IRPE_FUSED", None)
    print(json.dumps(dict(workload="DETR-with-iRPE encoder self-attention fwd+bwd, rpe-2.0-product-ctx-1-k, bf16 autocast, "
                                   "dropout 0.1, right third of image 1 padded", N=N, H=heads, head_dim=E // heads, L=Ld, hw=hw,
                          buckets=att.rpe_k.num_buckets, steps=steps, warmup=warmup, **res,
                          fused_over_composed=round(res["fused"]["median_ms"] / res["composed"]["median_ms"], 3))), flush=True)


if leg in ("all", "detr"):
    detr_leg()
