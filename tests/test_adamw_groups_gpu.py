"""cream_adamw_step_groups — the one-launch AdamW with one learning rate per parameter group — and NativeAdamW on top of it.

Kernel level, on the 11-job synthetic table of tests/test_ends_gpu.py (scalar and vector paths, a strided tensor,
de-interleaved tensors with a row tail inside a tile, a g == NULL job between updated ones, jobs of 1, 2, 4 and 9 tiles,
weight decay 0 and 0.05).  The rule: the grouped launch gives every job, BIT FOR BIT, what the ungrouped launch gives it when
run with that job's rate on a problem built from the same seed — the rate is the only thing a group changes; against float64
the yardstick is the existing one (ends_ref.check_against_fp32_baseline, baseline torch.optim.AdamW(foreach=False)).
The job -> group map is not monotonic, and the 9-tile job sits in another group than both neighbours (an index by tile or by
launch order would show)."""
import pytest
import torch

import ends_ref as R
from test_tinyvit_finetune import WarmupCosine, build
from test_ends_gpu import BETA1, BETA2, DEV, EPS, LR, NAN, SENT, Guarded, _AdamwProblem, _bits, _hold, _report

pytestmark = pytest.mark.gpu

GMAP = [(2, 0, 1)[i % 3] for i in range(11)]             # jobs 4, 5 (nine tiles), 6 -> groups 0, 1, 2
RATES = [LR, 1e3 * LR, 0.0]
BUFS = ("p", "m", "v", "mir", "mir_t")


def _grouped(table, gmap):
    """The same device jobs as `table`, as a JobTable built with a job -> group list."""
    from cream_amd import _lib as L
    from cream_amd.autoformer import block as K
    raw = table.jobs.cpu().numpy().tobytes()
    jobs = list((L.ParamJob * table.n).from_buffer_copy(raw))
    t = K.JobTable(jobs, torch.device(DEV), groups=gmap)
    assert t.total == table.total and t.groups.dtype == torch.int32 and t.groups.cpu().tolist() == list(gmap)
    return t


def _same_job(a, b, what=BUFS):
    """Every buffer of job dict a bit-identical to b's (bands and padding included)."""
    for k in what:
        if k in a and not torch.equal(_bits(a[k].whole), _bits(b[k].whole)):
            return k
    return None


def _launch(table, step, lr, coef=None, update=True):
    table.launch(update=update, lr=lr, beta1=BETA1, beta2=BETA2, eps=EPS, step=step, coef=coef)
    torch.cuda.synchronize()


def test_equal_rates_are_the_ungrouped_launch_bit_for_bit():
    a, b = _AdamwProblem(2, None), _AdamwProblem(2, None)
    tb = _grouped(b.table, GMAP)
    for step in (1, 2, 3):
        for pb in (a, b):
            pb.new_gradients()
            pb.poison_copies()
        _launch(a.table, step, LR)
        _launch(tb, step, [LR, LR, LR])
        for ja, jb in zip(a.jobs, b.jobs):
            assert _same_job(ja, jb) is None, (step, ja["name"], _same_job(ja, jb))
        b.check_untouched(("m", "v", "p"), padding_only=True)
        b.check_copies()


def test_distinct_rates_give_every_job_its_own_groups_rate_exactly():
    g = _AdamwProblem(5, None)
    tg = _grouped(g.table, GMAP)
    refs = [_AdamwProblem(5, None) for _ in RATES]
    assert GMAP[5] not in (GMAP[4], GMAP[6]) and GMAP != sorted(GMAP)
    for step in (1, 2):
        for pb in [g] + refs:
            pb.new_gradients()
            pb.poison_copies()
        before = [_bits(j["p"].whole).clone() for j in g.jobs]
        moments = [(_bits(j["m"].whole).clone(), _bits(j["v"].whole).clone()) for j in g.jobs]
        _launch(tg, step, RATES)
        for ref, rate in zip(refs, RATES):
            _launch(ref.table, step, rate)
        for i, jg in enumerate(g.jobs):
            bad = _same_job(jg, refs[GMAP[i]].jobs[i])
            assert bad is None, f"step {step} job {jg['name']} group {GMAP[i]}: {bad} differs from the ungrouped launch at its rate"
            for k, other in enumerate(refs):                         # ... and from the launches at the other rates
                if k != GMAP[i] and jg["has_g"] and jg["rows"] * jg["cols"] > 1:     # (the 1 x 1 job's only gradient is zero)
                    assert _same_job(jg, other.jobs[i], ("p",)) == "p", (jg["name"], k)
            if RATES[GMAP[i]] == 0.0 and jg["has_g"]:                    # lr = 0: p stays, the moments move (as in torch)
                assert torch.equal(_bits(jg["p"].whole), before[i]), jg["name"]
                assert jg["rows"] * jg["cols"] == 1 or not torch.equal(_bits(jg["m"].whole), moments[i][0]) and not torch.equal(_bits(jg["v"].whole), moments[i][1])
        g.check_untouched(("m", "v", "p"), padding_only=True)
        g.check_copies()
        # the references must keep the grouped problem's state for the next step: copy it over (same shapes, same seed)
        for i, jg in enumerate(g.jobs):
            for ref in refs:
                for k in ("p", "m", "v"):
                    ref.jobs[i][k].whole.copy_(jg[k].whole)


def _float64_steps(pb, table, steps, worst):
    """pb.step of tests/test_ends_gpu.py with one rate per job: the grouped launch against ends_ref.adamw_step run per job with
    its rate, the fp32 baseline being torch.optim.AdamW(foreach=False) with one group per job."""
    rate = [RATES[g] for g in GMAP]
    upd = [(j, r) for j, r in zip(pb.jobs, rate) if j["has_g"]]
    opt = torch.optim.AdamW([dict(params=[j["q"]], weight_decay=j["wd"], lr=r) for j, r in upd], lr=LR, betas=(BETA1, BETA2),
                            eps=EPS, foreach=False)
    for j, _ in upd:
        if j["q"] in pb.opt.state:                                       # given moments (the late step)
            opt.state[j["q"]] = pb.opt.state[j["q"]]
    for step in steps:
        pb.new_gradients()
        pb.poison_copies()
        before = [_bits(j["p"].whole).clone() for j in pb.jobs]
        _launch(table, step, RATES)
        opt.step()
        for j, b, r in zip(pb.jobs, before, rate):
            c, name = j["cols"], j["name"]
            if not j["has_g"]:
                assert torch.equal(_bits(j["p"].whole), b), f"{name}: a job without gradient was updated"
                continue
            j["ref"] = list(R.adamw_step(*([j["ref"][0], j["gr"]] + j["ref"][1:]), r, BETA1, BETA2, EPS, j["wd"], step))
            st = opt.state[j["q"]]
            for what, buf, fw, ref in (("p", j["p"], j["q"].detach(), j["ref"][0]), ("m", j["m"], st["exp_avg"], j["ref"][1]),
                                       ("v", j["v"], st["exp_avg_sq"], j["ref"][2])):
                _hold(f"adamw groups {what} @ {name} step {step}", buf.t[:, :c], fw, ref, floor="elem", worst=worst)
        pb.check_untouched(("m", "v", "p"), padding_only=True)
        pb.check_copies()


def test_distinct_rates_against_float64():
    """Steps 1..3 from zero moments and one step 1000 from given moments, rates {LR, 1e3 LR, 0} by group.
    Measured on the MI355X (ulp of each value, worst over jobs and steps; kernel / torch fp32): steps 1..3 p 2.68 / 2.68,
    m 1.17 / 0.98, v 2.02 / 1.99; step 1000 p 2.87 / 2.63, m 0.92 / 0.69, v 1.08 / 1.08."""
    worst = {}
    pb = _AdamwProblem(2, None)
    _float64_steps(pb, _grouped(pb.table, GMAP), (1, 2, 3), worst)
    _report("groups, steps 1..3", worst)
    worst = {}
    pb = _AdamwProblem(3, 999)
    _float64_steps(pb, _grouped(pb.table, GMAP), (1000,), worst)
    _report("groups, step 1000", worst)


def test_clipped_and_grouped_is_the_clipped_launch_at_the_jobs_rate():
    g = _AdamwProblem(6, 999)
    tg = _grouped(g.table, GMAP)
    refs = [_AdamwProblem(6, 999) for _ in RATES]
    for pb in [g] + refs:
        pb.new_gradients()
        pb.poison_copies()
    grads = [_bits(j["g"].whole).clone() for j in g.jobs]
    out = tg.clip_coef(1.0)
    norm, coef = float(out[0]), float(out[1])
    assert norm > 1.0 and 0.0 < coef < 1.0, (norm, coef)                 # (gradients of 1e3 among them)
    _launch(tg, 1000, RATES, coef=out[1:])
    for ref, rate in zip(refs, RATES):
        o = ref.table.clip_coef(1.0)
        assert torch.equal(_bits(o), _bits(out))
        _launch(ref.table, 1000, rate, coef=o[1:])
    for i, jg in enumerate(g.jobs):
        assert _same_job(jg, refs[GMAP[i]].jobs[i]) is None, jg["name"]
        assert torch.equal(_bits(jg["g"].whole), grads[i]), f"{jg['name']}: the gradient was scaled in memory"
    # ... and it is not the unclipped launch
    plain = _AdamwProblem(6, 999)
    plain.new_gradients()
    _launch(_grouped(plain.table, GMAP), 1000, RATES)
    assert _same_job(g.jobs[5], plain.jobs[5], ("p",)) == "p"


class _Flat:
    """A table of plain contiguous jobs, each with a row copy: shapes[i] = (rows, cols)."""

    def __init__(self, shapes, seed):
        from cream_amd.autoformer import block as K
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.jobs, self.cjobs = [], []
        for rows, cols in shapes:
            j = {k: Guarded((rows, cols)) for k in ("p", "g", "m", "v")}
            j["mir"] = Guarded((rows, cols), torch.bfloat16, fill=SENT)
            j["p"].t.copy_(0.5 + torch.rand(rows, cols, device=DEV, generator=gen))
            j["g"].t.copy_(0.1 * torch.randn(rows, cols, device=DEV, generator=gen))
            j["m"].t.copy_(0.01 * torch.randn(rows, cols, device=DEV, generator=gen))
            j["v"].t.copy_(1e-4 * (0.5 + torch.rand(rows, cols, device=DEV, generator=gen)))
            self.jobs.append(j)
            self.cjobs.append(K.param_job(j["p"].t, j["g"].t, j["m"].t, j["v"].t, j["mir"].t, None, weight_decay=0.05))

    def table(self, groups=None):
        from cream_amd.autoformer import block as K
        return K.JobTable(self.cjobs, torch.device(DEV), groups=groups)


def test_sixty_four_groups_and_the_copy_mode():
    """65 jobs in 64 groups (the limit): 64 one-tile jobs, one per group in a scrambled order, and the 9-tile job between them,
    which shares group 40 with a one-tile job far from it.  Rates LR (1 + k / 64); index 63 is used.  Groups 0, 1, 31, 62, 63
    and the 9-tile job are bit-identical to the ungrouped launch at their rate.  update = 0 through the grouped entry point:
    p, m, v untouched, every copy written."""
    shapes = [(1 + k % 5, 3 + k % 7) for k in range(64)]
    shapes.insert(20, (200, 130))
    gmap = [(37 * k + 5) % 64 for k in range(64)]                        # a permutation of 0..63 (37 is odd)
    assert sorted(gmap) == list(range(64)) and gmap.index(40) > 30
    gmap.insert(20, 40)
    rates = [LR * (1.0 + k / 64.0) for k in range(64)]
    g = _Flat(shapes, 11)
    tg = g.table(gmap)
    assert tg.total == 64 + 9
    _launch(tg, 7, rates)
    for grp in (0, 1, 31, 62, 63, 40):
        ref = _Flat(shapes, 11)
        _launch(ref.table(), 7, rates[grp])
        for i, gi in enumerate(gmap):
            same = _same_job(g.jobs[i], ref.jobs[i], ("p", "m", "v", "mir")) is None
            assert same == (gi == grp), (grp, i, gi)
    for j in g.jobs:
        assert all(j[k].intact() for k in ("p", "g", "m", "v", "mir"))
        assert torch.equal(_bits(j["mir"].t), _bits(j["p"].t.bfloat16()))
    # copy mode
    keep = [{k: _bits(j[k].whole).clone() for k in ("p", "m", "v")} for j in g.jobs]
    for j in g.jobs:
        j["mir"].t.fill_(NAN)
    _launch(tg, 1, rates, update=False)
    for j, b in zip(g.jobs, keep):
        assert all(torch.equal(_bits(j[k].whole), b[k]) for k in b)
        assert j["mir"].intact() and torch.equal(_bits(j["mir"].t), _bits(j["p"].t.bfloat16()))


def test_a_stored_group_index_one_past_the_end_takes_the_last_group():
    a, b = _AdamwProblem(8, None), _AdamwProblem(8, None)
    past = [3 if g == 2 else g for g in GMAP]                            # ngroups = 3: index 3 is one past the end
    for pb in (a, b):
        pb.new_gradients()
        pb.poison_copies()
    _launch(_grouped(a.table, GMAP), 1, RATES[:2] + [2 * LR])
    _launch(_grouped(b.table, past), 1, RATES[:2] + [2 * LR])
    for ja, jb in zip(a.jobs, b.jobs):
        assert _same_job(ja, jb) is None, ja["name"]
    b.check_untouched(("m", "v", "p"), padding_only=True)
    b.check_copies()


# ---- NativeAdamW --------------------------------------------------------------------------------------------------------
def _tinyvit():
    return build().to(DEV)


def _inject(models, gen, scale=0.1, away=False):
    """The same seeded gradient into the parameters of every model (copied into existing gradient tensors).  `away`: every
    element's sign is the opposite of its parameter's, so that the update moves the parameter away from zero and no element
    of p is the small difference of two large terms (as in the synthetic problem: an element-wise relative yardstick)."""
    for ps in zip(*[m.parameters() for m in models]):
        if away:
            gr = -torch.sign(ps[0].detach()) * scale * (0.5 + torch.rand(ps[0].shape, device=DEV, generator=gen))
        else:
            gr = torch.randn(ps[0].shape, device=DEV, generator=gen) * scale
        for p in ps:
            if p.grad is None:
                p.grad = gr.clone()
            else:
                p.grad.copy_(gr)


def test_native_adamw_with_the_recipes_groups_against_float64():
    """The small TinyViT with build_finetune_optimizer's ten groups (layer_lr_decay 0.8, base rate 1e-2), three steps on seeded
    gradients with the wrapped stand-in scheduler stepping in between, the second with max_norm: parameters and moments against
    the float64 AdamW run per parameter with its group's rate, baseline torch.optim.AdamW(foreach=False) on a twin.  The job
    table survives the changing rates and is rebuilt when the membership of the groups changes."""
    from cream_amd import tinyvit_finetune as FT
    from cream_amd.autoformer import engine
    m, twin = _tinyvit(), _tinyvit()
    opt = FT.build_finetune_optimizer(m, 1e-2)
    assert isinstance(opt, engine.NativeAdamW) and len(opt.param_groups) == 10
    ref_opt = torch.optim.AdamW(FT.finetune_param_groups(twin), lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-8, foreach=False)
    assert [g['weight_decay'] for g in opt.param_groups] == [g['weight_decay'] for g in ref_opt.param_groups]
    sched, ref_sched = (FT.LRSchedulerWrapper(WarmupCosine(o, 1e-2), o) for o in (opt, ref_opt))
    ref64 = {p: [p.detach().double(), torch.zeros_like(p).double(), torch.zeros_like(p).double()] for p in m.parameters()}
    gen = torch.Generator(device=DEV).manual_seed(7)
    worst, table = {}, None
    for step, max_norm in ((1, None), (2, 1.0), (3, None)):
        for s in (sched, ref_sched):
            s.step_update(step + 1)                                      # inside the warm-up: another rate every step
        rates = [g['lr'] for g in opt.param_groups]
        assert rates == [g['lr'] for g in ref_opt.param_groups] and len(set(rates)) == 5
        _inject((m, twin), gen, away=True)
        g64 = {p: p.grad.double() for p in m.parameters()}
        if max_norm is not None:
            norm64 = torch.sqrt(sum((g * g).sum() for g in g64.values()))
            coef64 = min(1.0, max_norm / (float(norm64) + 1e-6))
            assert coef64 < 1.0
            g64 = {p: g * coef64 for p, g in g64.items()}
            kept = [p.grad.clone() for p in m.parameters()]
            opt.step(max_norm=max_norm)
            assert all(torch.equal(p.grad, k) for p, k in zip(m.parameters(), kept))          # .grad stays unscaled
            assert abs(float(opt.grad_norm) - float(norm64)) <= 1e-5 * float(norm64)
            torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
        else:
            opt.step()
        ref_opt.step()
        torch.cuda.synchronize()
        table = table or opt._table
        assert opt._table is table, "a changed lr rebuilt the job table"
        for group, rate in zip(opt.param_groups, rates):
            for p in group['params']:
                ref64[p] = list(R.adamw_step(ref64[p][0], g64[p], ref64[p][1], ref64[p][2], rate, 0.9, 0.999, 1e-8,
                                             group['weight_decay'], step))
        for p, q in zip(m.parameters(), twin.parameters()):
            st, st_ref = opt.state[p], ref_opt.state[q]
            for what, got, fw, ref in (("p", p.detach(), q.detach(), ref64[p][0]), ("m", st["exp_avg"], st_ref["exp_avg"], ref64[p][1]),
                                       ("v", st["exp_avg_sq"], st_ref["exp_avg_sq"], ref64[p][2])):
                _hold(f"tinyvit groups {what} @ {p.param_name} step {step}", got, fw, ref, floor="elem", worst=worst)
    _report("tinyvit, ten groups", worst)
    assert opt._table.groups.cpu().tolist() == [k for k, g in enumerate(opt.param_groups) for _ in g['params']]
    # membership: a new group, then a parameter moved to another group
    extra = torch.nn.Parameter(torch.ones(5, 3, device=DEV))
    extra.grad = torch.full_like(extra, 0.5)
    opt.add_param_group(dict(params=[extra], lr=0.25))
    opt.step()
    assert opt._table is not table and opt._table.n == table.n + 1 and opt._table.groups.cpu().tolist()[-1] == 10
    torch.cuda.synchronize()
    # (step 4 from zero moments: bias corrections 1 - 0.9^4 and 1 - 0.999^4 on m = 0.1 g, v = 0.001 g^2)
    want = 1.0 - 0.25 * (0.1 * 0.5 / (1 - 0.9 ** 4)) / ((0.001 * 0.25 / (1 - 0.999 ** 4)) ** 0.5 + 1e-8)
    assert float((extra.detach() - want).abs().max()) <= 4 * 2.0 ** -24
    table = opt._table
    moved = opt.param_groups[0]['params'].pop()
    opt.param_groups[4]['params'].append(moved)
    opt.step()
    assert opt._table is not table and opt._table.groups.cpu().tolist().count(4) == len(opt.param_groups[4]['params'])
    torch.cuda.synchronize()


def _supernet_groups(model, lr, head_factor=10.0):
    from cream_amd.autoformer import engine
    head = {id(model.head.weight), id(model.head.bias)}
    groups = engine.param_groups(model, 0.05)
    out = [dict(g, params=[p for p in g['params'] if id(p) not in head], lr=lr) for g in groups]
    out += [dict(g, params=[p for p in g['params'] if id(p) in head], lr=head_factor * lr) for g in groups]
    assert all(g['params'] for g in out)
    return out


def test_supernet_with_two_rates_keeps_the_operand_copies_current():
    """engine.build_supernet("S", depth=2), the head at 10 x the rate of the rest (the jobs that come from ops.jobs(...): blocks,
    patch embedding, head): after two steps every block's copies equal bf16 of the kernel's own weights bit for bit, and the
    parameters stay within the existing test's bound of the torch twin."""
    from cream_amd.autoformer import block as K_, engine
    torch.manual_seed(3)
    m = engine.build_supernet("S", depth=2).to(DEV)
    ref = engine.build_supernet("S", depth=2).to(DEV)
    ref.load_state_dict(m.state_dict())
    lr = 2e-2 * 128 / 512
    opt = engine.NativeAdamW(m, _supernet_groups(m, lr), lr=lr)
    opt_ref = torch.optim.AdamW(_supernet_groups(ref, lr), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    gen = torch.Generator(device=DEV).manual_seed(7)
    for _ in range(2):
        _inject((m, ref), gen)
        opt.step()
        opt_ref.step()
    assert sorted(set(opt._table.groups.cpu().tolist())) == [0, 1, 2, 3]
    worst = 0.0
    for p, q in zip(m.parameters(), ref.parameters()):
        worst = max(worst, float((p.detach() - q.detach()).abs().max() / (q.detach().abs().max() + 1e-12)))
    assert worst < 2e-6, worst
    moved = float((m.head.weight - ref.head.weight).detach().abs().max()), float(ref.head.weight.detach().abs().max())
    assert moved[0] < 2e-6 * moved[1]
    for blk in m.blocks:
        ops = K_.operands(blk, fresh=False)
        assert not ops.stale()
        for mod, w, wt, b in zip(ops.mods, ops.w, ops.wt, ops.b):
            W = mod.weight.detach().bfloat16()
            if w.dim() == 3:
                W = torch.stack([W[i::3] for i in range(3)])
            assert torch.equal(w, W) and torch.equal(wt, W.transpose(-1, -2))
            assert torch.equal(b, mod.bias.detach().bfloat16())


def test_equal_rates_take_the_old_entry_point(monkeypatch):
    from cream_amd import _lib as L
    from cream_amd import tinyvit_finetune as FT
    from cream_amd.autoformer import block as K_
    m = _tinyvit()
    opt = FT.build_finetune_optimizer(m, 1e-2)
    _inject((m,), torch.Generator(device=DEV).manual_seed(1))
    seen, entries = [], []
    launch = K_.JobTable.launch
    monkeypatch.setattr(K_.JobTable, "launch", lambda self, **kw: (seen.append(kw["lr"]), launch(self, **kw))[1])
    lib = L.load()
    for name in ("cream_adamw_step", "cream_adamw_step_clipped", "cream_adamw_step_groups"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (entries.append(_n), _fn(*a))[1])
    opt.step()
    opt.step(max_norm=1.0)
    assert seen == [1e-2, 1e-2] and all(type(v) is float for v in seen)
    assert entries == ["cream_adamw_step", "cream_adamw_step_clipped"]
    opt.param_groups[3]['lr'] = 5e-3
    opt.step()
    opt.step(max_norm=1.0)
    assert seen[2] == seen[3] == [1e-2] * 3 + [5e-3] + [1e-2] * 6
    assert entries[2:] == ["cream_adamw_step_groups", "cream_adamw_step_groups"]
    torch.cuda.synchronize()


def test_error_paths():
    from cream_amd.autoformer import engine
    ps = torch.nn.ParameterList([torch.nn.Parameter(torch.ones(3, device=DEV)) for _ in range(65)])
    opt = engine.NativeAdamW(ps, [dict(params=[p], weight_decay=0.0) for p in ps], lr=1e-3)
    with pytest.raises(ValueError, match="64"):
        opt.step()
    for key, other in (("betas", (0.8, 0.999)), ("eps", 1e-6)):
        opt = engine.NativeAdamW(ps, [dict(params=list(ps)[:30], weight_decay=0.0), dict(params=list(ps)[30:], weight_decay=0.0)],
                                 lr=1e-3)
        opt.step()                                                       # equal: fine
        opt.param_groups[1][key] = other
        with pytest.raises(ValueError, match="betas and eps"):
            opt.step()
    torch.cuda.synchronize()


def test_state_dict_round_trip_into_torch_adamw():
    from cream_amd import tinyvit_finetune as FT
    m = _tinyvit()
    opt = FT.build_finetune_optimizer(m, 1e-2)
    for k, g in enumerate(opt.param_groups):
        g['lr'] = 1e-2 * g['lr_scale']
    gen = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(2):
        _inject((m,), gen)
        opt.step()
    sd = opt.state_dict()
    assert [g['lr_scale'] for g in sd['param_groups']] == [g['lr_scale'] for g in opt.param_groups]
    t = torch.optim.AdamW(FT.finetune_param_groups(m), lr=1e-2, weight_decay=1e-8)
    t.load_state_dict(sd)
    assert [g['lr_scale'] for g in t.param_groups] == [g['lr_scale'] for g in opt.param_groups]
    assert [g['lr'] for g in t.param_groups] == [g['lr'] for g in opt.param_groups]
    for p in m.parameters():
        assert torch.equal(t.state[p]['exp_avg'], opt.state[p]['exp_avg']) and torch.equal(t.state[p]['exp_avg_sq'], opt.state[p]['exp_avg_sq'])
        assert int(t.state[p]['step']) == 2
    opt2 = FT.build_finetune_optimizer(m, 1e-2)
    opt2.load_state_dict(sd)
    assert opt2._steps == 2 and [g['lr_scale'] for g in opt2.param_groups] == [g['lr_scale'] for g in opt.param_groups]
    p = next(iter(m.parameters()))
    assert torch.equal(opt2.state[p]['exp_avg'], opt.state[p]['exp_avg'])
    _inject((m,), gen)
    opt2.step()                                                          # (the table is rebuilt on the loaded moments)
    torch.cuda.synchronize()
    assert opt2._steps == 3
