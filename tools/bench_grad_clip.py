"""Global-norm gradient clipping on the device (csrc/optim.hip: grad_sqnorm_kernel + grad_norm_finish_kernel, the clipped
AdamW launch, grad_scale_kernel): kernel-level times on the supernet-S job table of engine.build_optimizer and the cost of
clipping inside SupernetTrainer.step at per-GPU batch 128.  Device events, warm, legs alternating inside ONE process (the same-call
A/B convention); needs the GPU and fails without one.

    python tools/bench_grad_clip.py [--iters 200] [--batch 128] [--no-step] > grad_clip.json
"""
import argparse
import json
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cream_amd.autoformer import engine

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--no-step", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_grad_clip needs the MI355X: there is no other path to measure")
dev = torch.device("cuda:0")
torch.manual_seed(0)
COPY_TBS = 4.7                               # the device-to-device copy figure this project sees, TB/s


def stats(ms):
    s = sorted(ms)
    return dict(median_us=round(statistics.median(s) * 1e3, 2), mean_us=round(statistics.fmean(s) * 1e3, 2),
                p10_us=round(s[len(s) // 10] * 1e3, 2), p90_us=round(s[(9 * len(s)) // 10] * 1e3, 2), n=len(s))


def timed_rounds(legs, rounds, inner):
    """legs: name -> callable.  Every round runs each leg `inner` times between two events, legs in turn; ms per call."""
    out = {k: [] for k in legs}
    for r in range(rounds + 2):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if r >= 2:                       # two warm rounds
                out[k].append(e0.elapsed_time(e1) / inner)
    return out


model = engine.build_supernet("S").to(dev)
opt = engine.build_optimizer(model, batch_size=a.batch)
g = torch.Generator(device=dev).manual_seed(1)
for p in model.parameters():
    p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-2
opt._build()
table = opt._table
n_elem = sum(p.numel() for p in model.parameters())
hp = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)
counter = [0]


def adamw(coef=None):
    counter[0] += 1
    table.launch(update=True, step=counter[0], coef=coef, **hp)


out = table.clip_coef(5.0)
torch.cuda.synchronize()
norm0 = float(out[0])
c_lt1 = torch.tensor([0.999], device=dev)    # (scaling in place 200 x 10 times: stays far from the denormals)
c_one = torch.ones(1, device=dev)
legs = {
    "reduction (grad_sqnorm + grad_norm_finish)": lambda: table.clip_coef(5.0),
    "cream_adamw_step": lambda: adamw(),
    "cream_adamw_step_clipped": lambda: adamw(out[1:]),
    "cream_grad_scale c<1": lambda: table.scale_grads(c_lt1),
    "cream_grad_scale c==1": lambda: table.scale_grads(c_one),
}
INNER = 10
res = {k: stats(v) for k, v in timed_rounds(legs, max(a.iters // INNER, 20), INNER).items()}
for k, nbytes in (("reduction (grad_sqnorm + grad_norm_finish)", 4 * n_elem), ("cream_grad_scale c<1", 8 * n_elem)):
    res[k]["bytes"] = nbytes
    res[k]["TB_per_s"] = round(nbytes / (res[k]["median_us"] * 1e-6) / 1e12, 3)
    res[k]["fraction_of_copy_figure"] = round(res[k]["TB_per_s"] / COPY_TBS, 3)
line = dict(workload="gradient clipping kernels on the supernet-S job table", jobs=table.n, tiles=table.total, parameters=n_elem,
            grad_norm=norm0, launches_per_timed_interval=INNER, copy_figure_TB_per_s=COPY_TBS, kernels=res)

if not a.no_step:
    # ---- step level: (a) no clipping, (b) max_norm = 5 on the new path, (c) the framework's clip_grad_norm_ + step() ----------
    B = a.batch
    x = torch.randn(B, 3, 224, 224, device=dev, generator=g)
    t = torch.softmax(torch.randn(B, 1000, device=dev, generator=g), -1)
    tr = engine.SupernetTrainer(model, opt, engine.SEARCH_SPACES["S"]["choices"])
    tr.start_epoch(0)

    def leg_a():
        tr.max_norm = 0.0
        tr.step(x, t)

    def leg_b():
        tr.max_norm = 5.0
        tr.step(x, t)

    def leg_c():                             # SupernetTrainer.step as it was before the clip kernels
        tr.sample()
        tr.forward_backward(x, t)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
        opt.step()

    step_legs = {"a: max_norm=None": leg_a, "a again (spread)": leg_a, "b: max_norm=5, clip kernels": leg_b,
                 "c: framework clip_grad_norm_ + step()": leg_c}
    times = {k: [] for k in step_legs}
    for r in range(a.iters + 5):
        state = random.getstate()
        for k, fn in step_legs.items():
            random.setstate(state)           # the same sub-network for every leg of a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= 5:
                times[k].append(e0.elapsed_time(e1))
        random.setstate(state)
        tr.sample()                          # move on to the next sub-network
    sres = {k: dict(median_ms=round(statistics.median(v), 4), mean_ms=round(statistics.fmean(v), 4), n=len(v)) for k, v in times.items()}
    # paired differences per round (same sub-network): the noise of a step cancels
    def paired(k1, k2):
        d = [p - q for p, q in zip(times[k1], times[k2])]
        return dict(median_ms=round(statistics.median(d), 4), mean_ms=round(statistics.fmean(d), 4))
    line["step"] = dict(workload=f"SupernetTrainer.step, supernet-S, batch {B}, bf16, one event pair per step (host waits for each step)",
                        legs=sres,
                        paired=dict(a_again_minus_a=paired("a again (spread)", "a: max_norm=None"),
                                    b_minus_a=paired("b: max_norm=5, clip kernels", "a: max_norm=None"),
                                    c_minus_a=paired("c: framework clip_grad_norm_ + step()", "a: max_norm=None"),
                                    b_minus_c=paired("b: max_norm=5, clip kernels", "c: framework clip_grad_norm_ + step()")))
print(json.dumps(line))
