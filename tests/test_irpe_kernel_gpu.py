"""The kernels of csrc/irpe_attn.hip and csrc/irpe_attn_x.hip, called directly (`fwd_core` / `bwd_core`, `fwd_core_x` /
`bwd_core_x`), against the fp64 CPU reference of tests/irpe_ref.py — every element of every returned tensor (out, lse, delta,
dq, dk, dv, each table gradient, the side rows sv, lkg, gg, dlk, dlq, and what the table-gradient kernels add to the rows they
are handed) under the per-element bound derived there from the kernels' rounding points.  The case lists turn every loop and
dispatch: L around the 32-token tile and the 128-token workgroup, every subset of q / k / v, shared and per-head tables,
bucket counts at 51 | 52, 64 | 65 and 128 from hand-built tables with independent, non-symmetric id matrices, bias mode,
real modules, dropout, causal, and for the x family both head dims and row widths, six key padding patterns and the three
operand layouts.  tests/test_irpe_ref_cpu.py proves the method on the CPU."""
import copy

import pytest
import torch

import irpe_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _timed(fn):
    from cream_amd import timing
    timing.reset()
    timing.enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        timing.enable(False)
    return res, set(timing.summary())


def _terms(o):
    """The tuples `irpe_fused._term` returns: from the real module where the case has one, built by hand otherwise."""
    from cream_amd import irpe_fused
    c = o.case
    out = []
    for t in o.terms:
        if t is None:
            out.append(None)
        elif t.module is not None:
            out.append(irpe_fused._term(copy.deepcopy(t.module).to(DEV), c.L, torch.device(DEV), c.hw))
            assert out[-1][4] == t.nb and out[-1][5] == t.bias and torch.equal(out[-1][0].detach().cpu(), t.table)
        else:
            w = t.table.to(DEV).contiguous()
            asis, tr = irpe_fused.bucket_bytes(t.ids.to(torch.int32).to(DEV).contiguous())
            out.append((w, 0 if w.shape[0] == 1 else w[0].numel(), asis, tr, t.nb, t.bias))
    return tuple(out)


def run(c):
    """-> ({name: CPU tensor in the layout of R.reference}, timing regions seen)"""
    from cream_amd import irpe_fused
    o = R.operands(c)
    B, H, L, D = c.B, c.H, c.L, c.D
    NP, W = R.padded_len(L), R.row_width_of(c)
    terms = _terms(o)
    assert irpe_fused.row_width(terms) == W
    qkv, dout = o.qkv.to(DEV), o.dout.to(DEV)
    kw = dict(drop_p=c.drop, seed=o.seed, causal=c.causal)
    seq_first = c.layout == "seqfirst"
    if c.fam == "base":                                      # csrc/irpe_attn.hip: the packed entry, 64-wide rows
        assert D == 64 and W == 64 and c.mask is None and c.layout == "packed"

        def go():
            out, lse, sv = irpe_fused.fwd_core(qkv, c.scale, terms, **kw)
            dqkv, res, rows = irpe_fused.bwd_core(dout, qkv, out, lse, sv, c.scale, terms, **kw, return_rows=True)
            return out, lse, sv, (dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]), res, rows
    else:                                                    # csrc/irpe_attn_x.hip
        pad = irpe_fused._pad_bytes(o.pad.to(DEV), B, L) if o.pad is not None else None
        if c.layout == "packed":
            q, k, v = (qkv[:, :, i] for i in range(3))
        elif c.layout == "separate":
            q, k, v = (qkv[:, :, i].contiguous() for i in range(3))
        else:                                                # (L, B, H, D) buffers viewed as (B, L, H, D)
            q, k, v = (qkv[:, :, i].permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3) for i in range(3))
            dout = dout.permute(1, 0, 2).contiguous()
        assert q.stride() == k.stride() == v.stride()

        def go():
            out, lse, sv = irpe_fused.fwd_core_x(q, k, v, c.scale, terms, pad, **kw, seq_first=seq_first)
            d3, res, rows = irpe_fused.bwd_core_x(dout, q, k, v, out, lse, sv, c.scale, terms, pad, **kw, seq_first=seq_first,
                                                  return_rows=True)
            return out, lse, sv, d3, res, rows

    (out, lse, sv, d3, res, rows), names = _timed(go)
    assert out.dtype == torch.bfloat16 and out.shape == ((L, B, H * D) if seq_first else (B, L, H * D))
    assert lse.shape == (B, H, L) and lse.dtype == torch.float32 and rows["delta"].shape == (B, H, NP)
    assert all(t.dtype == torch.bfloat16 and t.shape == (B, L, H, D) for t in d3)
    heads = lambda t: t.permute(0, 2, 1, 3)                  # noqa: E731  (B, L, H, D) -> (B, H, L, D)
    out4 = out.view(L, B, H, D).permute(1, 0, 2, 3) if seq_first else out.view(B, L, H, D)
    got = {"out": heads(out4), "lse": lse, "delta": rows["delta"][:, :, :L], "dq": heads(d3[0]), "dk": heads(d3[1]), "dv": heads(d3[2])}
    rows = dict(rows, sv=sv)
    for name, t, g in zip(R.TABLES, o.terms, res):
        assert (g is None) == (t is None)
        if t is not None:
            assert g.shape == t.table.shape and g.dtype == torch.float32
            got[name] = g
    for name, t in (("sv", o.terms[2]), ("lkg", o.terms[1]), ("gg", o.terms[2]), ("dlk", o.terms[1]), ("dlq", o.terms[0])):
        assert (rows[name] is None) == (t is None), name
        if t is not None:
            assert rows[name].shape == (B, H, NP, W) and rows[name].dtype == torch.bfloat16
            got[name] = rows[name][:, :, :L, :t.nb]
    got = {n: t.detach().cpu() for n, t in got.items()}
    got.update(R.residuals(o, got, True))
    return got, names


FP32 = ("lse", "delta") + R.TABLES + R.RESIDUALS


def _compare(case, got, ref, bound):
    tag = R.cid(case)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = {n: R.worst_ratio(got[n], ref[n], bound[n]) for n in ref}
    print(f"[irpe kernel {tag}] error / bound: " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    centre, slack = R.centre_and_slack(case)                 # the fp32 tensors without the known shift of the lookup roundings
    print(f"[irpe kernel {tag}] fp32 error / slack: " + "  ".join(f"{n} {R.worst_ratio(got[n], centre[n], slack[n]):.3f}" for n in FP32 if n in got))
    bad = {n: v for n, v in worst.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("case", R.BASE_CASES + R.X_CASES, ids=R.cid)
def test_kernels_against_fp64(case):
    ref, bound = R.ref_and_bound(case)
    got, names = run(case)
    assert {"irpe_attn_fwd", "irpe_attn_bwd"} <= names, names
    o = R.operands(case)
    if o.pad is not None and bool(o.pad.any()):              # padded keys receive exactly 0
        m = o.pad[:, None, :, None].expand_as(got["dk"])
        assert not bool(got["dk"][m].any()) and not bool(got["dv"][m].any())
        if "dlq" in got:
            assert not bool(got["dlq"][o.pad[:, None, :, None].expand_as(got["dlq"])].any())
    _compare(case, got, ref, bound)


@pytest.mark.parametrize("which", ["base-len-L129", "base-drop0.5-L129", "x-d32w128-k81-L129", "x-drop-mask"])
def test_reruns_are_bit_identical(which):
    case = next(c for c in R.BASE_CASES + R.X_CASES if R.cid(c) == which)
    a, _ = run(case)
    b, _ = run(case)
    for n in a:
        assert torch.equal(a[n], b[n]), n
