"""The method of tests/window_xl_ref.py, proven without a GPU:
A. the per-window fp64 reference equals the fp64 autograd statement of attn_mix_ref.window_reference, and the hand-written
   arithmetic without roundings equals the reference (so the bound, computed from its intermediates, is a bound around it),
B. with the kernels' bf16 roundings the model stays inside the bound at every element of every tensor of every case,
C. each injected fault breaks the bound on every case it changes, and changes some,
D. the padded-key rule: the result does not depend on what the rows past N hold,
E. the case list covers what it claims, and the C ABI's argument check answers without a device."""
import ctypes

import pytest
import torch

import attn_mix_ref
import window_xl_ref as R


def test_case_list_covers_what_it_claims():
    C = R.XL_CASES
    assert len(set(C)) == len(C) and R.MANY_CASE not in C
    size = [c for c in C if c.group == "size"]
    assert [c.w for c in size] == [15, 16, 17, 24, 31, 32] and [R.np_of(c) // 32 for c in size] == [8, 8, 10, 18, 31, 32]
    assert 256 - 225 == 31 and 289 - 288 == 1 and 992 - 961 == 31                       # padded keys at 15 and 31, real ones at 17
    assert all((c.Hs, c.Ws) == (c.w, c.w) for c in size)
    assert {(c.H, c.w, c.B) for c in C if c.group == "heads"} == {(1, 17, 2), (32, 16, 1)}
    assert all(c.H != 32 or (c.w, c.B) == (16, 1) for c in C)
    assert {(c.Hs // c.w, c.Ws // c.w) for c in C if c.group == "map"} == {(2, 1), (1, 3)}
    assert {c.B for c in C} == {1, 2} and {c.H for c in C} == {1, 2, 3, 32}
    assert {c.scale for c in C} == {32 ** -0.5, 0.25}
    m = R.MANY_CASE
    assert m.w == 16 and m.H == 2 and m.B * (m.Hs // m.w) * (m.Ws // m.w) == 36
    for c in C + [m]:
        assert bool((R.xl_operands(c).table != 0).all()), c                             # a nonzero table everywhere
        assert c.Hs % c.w == 0 and c.Ws % c.w == 0


@pytest.mark.parametrize("case", [c for c in R.XL_CASES if c.w <= 17 and c.H <= 3], ids=R.xid)
def test_reference_equals_the_autograd_statement(case):
    o = R.xl_operands(case)
    mine, auto = R.xl_reference(o), attn_mix_ref.window_reference(o)
    assert set(mine) == set(auto)
    for n in mine:
        scale = float(auto[n].abs().max()) + 1e-300
        assert mine[n].shape == auto[n].shape and float((mine[n] - auto[n]).abs().max()) <= 1e-10 * scale, n


@pytest.mark.parametrize("case", R.XL_CASES + [R.MANY_CASE], ids=R.xid)
def test_rounding_model_lies_inside_the_bound(case):
    o = R.xl_operands(case)
    ref, bound = R.xl_ref_and_bound(case)
    plain, model = R.xl_model(o, rounded=False), R.xl_model(o, rounded=True)
    assert set(plain) == set(ref) == set(bound)
    worst = {}
    for n in ref:
        scale = float(ref[n].abs().max()) + 1e-300
        assert float((plain[n] - ref[n]).abs().max()) <= 1e-9 * scale, (n, float((plain[n] - ref[n]).abs().max()), scale)   # A
        assert bound[n].shape == ref[n].shape and bool((bound[n] > 0).all()), n
        worst[n] = R.worst_ratio(model[n], ref[n], bound[n])
    print(f"[window_xl cpu {R.xid(case)}] " + "  ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst                                    # B


@pytest.mark.parametrize("fault", R.XL_FAULTS)
def test_injected_faults_leave_the_bound_on_every_case_they_change(fault):
    changed, missed = [], {}
    for c in R.XL_CASES:
        ref, bound = R.xl_ref_and_bound(c)
        faulty = R.xl_reference(R.xl_operands(c), fault)
        if all(torch.equal(faulty[n], ref[n]) for n in ref):
            continue
        changed.append(R.xid(c))
        ratios = {n: R.worst_ratio(faulty[n], ref[n], bound[n]) for n in ref}
        if not any(v > 1.0 for v in ratios.values()):
            missed[R.xid(c)] = ratios
    print(f"[window_xl sensitivity {fault}] changes {len(changed)} of {len(R.XL_CASES)} cases")
    assert changed and not missed, (fault, missed)
    if fault == "padding_counted":                            # exact tiles have no padding to count
        assert not any("-w16-" in x or "-w32-" in x for x in changed) and any("-w15-" in x for x in changed)


@pytest.mark.parametrize("case", [c for c in R.XL_CASES if c.w in (15, 17, 31) and c.group == "size"], ids=R.xid)
def test_padded_keys_contribute_exactly_nothing(case):
    o = R.xl_operands(case)
    plain = R.xl_model(o, rounded=False)
    for garbage in (0.0, 1e4, -3.0):
        padded = R.xl_model(o, rounded=False, garbage=garbage)
        for n in plain:
            scale = float(plain[n].abs().max()) + 1e-300
            assert float((padded[n] - plain[n]).abs().max()) <= 1e-12 * scale, (n, garbage)
    a, b = R.xl_model(o, rounded=True, garbage=1e4), R.xl_model(o, rounded=True, garbage=-3.0)
    assert all(torch.equal(a[n], b[n]) for n in a)            # the same padded arithmetic, different garbage: the same bits


def _desc(**kw):
    from cream_amd import _lib
    d = _lib.WindowAttnXlDesc()
    d.q, d.k, d.v, d.out, d.lse, d.table = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    d.sb, d.sn, d.sh = 576 * 288, 288, 32
    d.B, d.H, d.Hs, d.Ws, d.w, d.shift, d.mask_shift, d.head_dim = 2, 3, 24, 24, 24, 0, 0, 32
    d.scale = 32 ** -0.5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_c_abi_argument_checks_return_codes_without_a_launch():
    from cream_amd import _lib
    lib = _lib.load()
    ok = lambda d, bwd=0: lib.cream_window_attn_xl_check(ctypes.byref(d), bwd)          # noqa: E731
    assert ok(_desc()) == 0
    assert lib.cream_window_attn_xl_check(None, 0) == -1
    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(lse=None), dict(table=None),
                dict(head_dim=64), dict(w=14, Hs=28, Ws=28), dict(w=33, Hs=33, Ws=33), dict(w=0), dict(Hs=25), dict(Ws=36), dict(Hs=0),
                dict(shift=1), dict(shift=12), dict(shift=-1), dict(mask_shift=1), dict(H=0), dict(H=33), dict(B=-1), dict(sn=284),
                dict(q=0x1008)):
        d = _desc(**bad)
        assert ok(d) == -1, bad
        assert lib.cream_window_attn_xl_fwd(ctypes.byref(d), None) == -1, bad         # the same check, before any HIP call
        assert lib.cream_window_attn_xl_bwd(ctypes.byref(d), None) == -1, bad
    for w in range(15, 33):
        assert ok(_desc(w=w, Hs=w, Ws=2 * w)) == 0, w
    assert ok(_desc(H=32, sn=3 * 32 * 32, sb=576 * 3 * 32 * 32)) == 0 and ok(_desc(H=1)) == 0
    assert ok(_desc(w=16, Hs=64, Ws=64)) == 0 and ok(_desc(w=32, Hs=32, Ws=32)) == 0
    full = dict(dout=0x8000, dq=0x9000, dk=0xa000, dv=0xb000, dsb=576 * 288, dsn=288, dsh=32, delta=0xc000, part=0xd000, part_blocks=4)
    assert ok(_desc(**full), 1) == 0 and ok(_desc(), 1) == -1
    for k in ("dout", "dq", "dk", "dv", "delta", "part"):
        assert ok(_desc(**{**full, k: None}), 1) == -1, k
    assert ok(_desc(**{**full, "part_blocks": 0}), 1) == -1
    # an empty batch is a no-op success, forward and backward, and launches nothing
    assert lib.cream_window_attn_xl_fwd(ctypes.byref(_desc(B=0)), None) == 0
    assert lib.cream_window_attn_xl_bwd(ctypes.byref(_desc(B=0, **full)), None) == 0
    assert lib.cream_window_attn_xl_part_size(3, 24) == 47 * 47 * 3 and lib.cream_window_attn_xl_part_size(32, 32) == 3969 * 32
    assert lib.cream_window_attn_xl_part_size(3, 14) == -1 and lib.cream_window_attn_xl_part_size(3, 33) == -1
    assert lib.cream_window_attn_xl_part_size(0, 24) == -1 and lib.cream_window_attn_xl_part_size(33, 24) == -1


def test_host_constants_and_usable_truth_table(monkeypatch):
    from cream_amd import window_attn_large, window_attn_xl as W
    monkeypatch.delenv("CREAM_IRPE_FUSED", raising=False)
    assert (W.MIN_WINDOW, W.MAX_WINDOW, W.MAX_HEADS, W.HEAD_DIM) == (15, 32, 32, 32) and W.MIN_WINDOW == window_attn_large.MAX_WINDOW + 1
    assert [W.padded_tokens(w) for w in (15, 16, 17, 24, 31, 32)] == [256, 256, 320, 576, 992, 1024]
    bf, dev = torch.bfloat16, "cuda:0"
    table = lambda w, H: torch.zeros((2 * w - 1) ** 2, H)                                # noqa: E731
    assert W.usable_xl_window(bf, dev, 32, 12, 24, table(24, 12)) and W.usable_xl_window(bf, dev, 32, 32, 32, table(32, 32))
    assert W.usable_xl_window(bf, dev, 32, 1, 15, table(15, 1))
    assert not W.usable_xl_window(bf, dev, 32, 3, 14, table(14, 3)) and not W.usable_xl_window(bf, dev, 32, 3, 33, table(33, 3))
    assert not W.usable_xl_window(torch.float32, dev, 32, 3, 16, table(16, 3)) and not W.usable_xl_window(bf, "cpu", 32, 3, 16, table(16, 3))
    assert not W.usable_xl_window(bf, dev, 64, 3, 16, table(16, 3)) and not W.usable_xl_window(bf, dev, 32, 33, 16, table(16, 33))
    assert not W.usable_xl_window(bf, dev, 32, 3, 16, table(16, 3), dropout_p=0.1)
    assert not W.usable_xl_window(bf, dev, 32, 3, 16, None) and not W.usable_xl_window(bf, dev, 32, 3, 16, table(16, 3).double())
    assert not W.usable_xl_window(bf, dev, 32, 3, 16, table(16, 4)) and not W.usable_xl_window(bf, dev, 32, 3, 16, table(16, 6)[:, ::2])
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")
    assert not W.usable_xl_window(bf, dev, 32, 12, 24, table(24, 12))
