"""The Mini-Swin distillation step (cream_amd/minivit_distill.py, the distilling models of cream_amd/miniswin.py) without a
device, against fixtures made by running the reference's own classes and loss functions
(tests/golden/make_minivit_distill_golden.py): state-dict keys and shapes, the four return shapes, layer-id selection, logits,
the losses and the gradient of every student parameter on the composed fp32 path; the taps; `usable_*` truth tables; the
C ABI's argument checks."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from helpers import load_json, load_npz, max_rel  # noqa: E402
from make_minivit_distill_golden import LAYERS, SEEDS, SETTINGS, STUDENT, TEACHER, inputs, miniswin_fill  # noqa: E402
from make_miniswin_golden import STRIDE  # noqa: E402

TOL = 1e-5
_FIX = {}


def fixture():
    if not _FIX:
        _FIX.update(load_npz("minivit_distill.npz"))
    return _FIX


def build_pair(device="cpu"):
    from cream_amd import miniswin
    torch.manual_seed(0)
    student = miniswin.SwinTransformerMiniViTDistill(**STUDENT)
    teacher = miniswin.SwinTransformerDistill(**TEACHER)
    miniswin_fill(student, seed=SEEDS["student"])
    miniswin_fill(teacher, seed=SEEDS["teacher"])
    return student.eval().to(device), teacher.eval().to(device)


def config(org, **kw):
    from cream_amd.minivit_distill import DistillConfig
    return DistillConfig(student_layers=LAYERS, teacher_layers=LAYERS, hidden_relation=org, **kw)


def digest_errors(tag, grads):
    """-> {name: error} of gradient digests against the fixture: the norm relatively, the strided sample on the tensor's own
    scale (as tests/test_miniswin.py does)."""
    fix, errs = fixture(), {}
    for k, v in fix.items():
        if k.startswith(tag + "|") and k.endswith("|norm"):
            name = k[len(tag) + 1:-5]
            ref = float(v[0])
            g = grads[name].detach().cpu().double().flatten()
            if ref < 1e-5:
                errs[name + "|zero"] = float(g.norm())
                continue
            errs[name + "|norm"] = abs(float(g.norm()) - ref) / ref
            scale = ref / max(1.0, g.numel()) ** 0.5
            errs[name + "|sample"] = float((g[::STRIDE] - torch.from_numpy(fix[f"{tag}|{name}|sample"])).abs().max() / scale) / 10.0
    return errs


@pytest.fixture(scope="module")
def pair():
    return build_pair()


def test_state_dicts_match_the_reference(pair):
    meta = load_json("minivit_distill.json")
    for name, model in zip(("student", "teacher"), pair):
        sd = model.state_dict()
        assert list(sd.keys()) == meta[name]["keys"], name
        assert [list(v.shape) for v in sd.values()] == meta[name]["shapes"], name
        assert sum(p.numel() for p in model.parameters()) == meta[name]["n_params"], name
    s, t = (m.state_dict() for m in pair)
    assert tuple(s["fit_dense_C.1.weight"].shape) == (192, 128) and not any(k.startswith("fit_dense_C") for k in t)
    # the plain Swin: unshared blocks under the plain names, a mask on the shifted block only
    assert "layers.0.blocks.1.attn_mask" in t and "layers.0.blocks.0.attn_mask" not in t and "layers.0.blocks.1.norm1.weight" in t


def test_forward_has_the_four_return_shapes(pair):
    student, _ = pair
    x = inputs("distill")[0]
    with torch.no_grad():
        a = student(x)
        b = student(x, LAYERS, is_attn_loss=True)
        c = student(x, LAYERS, is_hidden_loss=True, is_hidden_org=False)
        d = student(x, LAYERS, is_attn_loss=True, is_hidden_loss=True)
    assert torch.is_tensor(a) and a.shape == (2, 1000)
    assert len(b) == 2 and len(c) == 2 and len(d) == 3
    assert torch.equal(b[0], a) and torch.equal(c[0], a) and torch.equal(d[0], a)
    shapes = load_json("minivit_distill.json")["tap_shapes"]
    assert [list(t[0].shape) for t in b[1]] == shapes["hidden_org"]["qkv"] and all(len(t) == 3 for t in b[1])
    assert [list(h.shape) for h in c[1]] == shapes["hidden_fit"]["hidden"]              # through fit_dense_C
    assert [list(h.shape) for h in d[2]] == shapes["hidden_org"]["hidden"]


def test_layer_ids_count_repeats_across_stages(pair):
    student, teacher = pair
    x = inputs("distill")[0]
    with torch.no_grad():
        for model, widths in ((student, [64, 64, 128, 128]), (teacher, [96, 96, 192, 192])):
            _, taps, hidden = model(x, [0, 1, 2, 3], is_attn_loss=True, is_hidden_loss=True, is_hidden_org=True)
            assert [t[0].shape[2] for t in taps] == widths and [h.shape[1] for h in hidden] == [196, 196, 49, 49]
            for ids in ([2], [1, 2], [3, 0], []):
                _, sel, hid = model(x, ids, is_attn_loss=True, is_hidden_loss=True, is_hidden_org=True)
                assert len(sel) == len(ids)
                for got, want in zip(sel, sorted(ids)):                                   # in layer order, whatever the list's
                    assert torch.equal(got[0], taps[want][0]) and torch.equal(got[2], taps[want][2])
                for got, want in zip(hid, sorted(ids)):
                    assert torch.equal(got, hidden[want])
    # the hidden state is the block's output BEFORE patch merging: stage one's last tap still has 196 tokens of width 64
    assert hidden[1].shape == (2, 196, 96)


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_losses_and_gradients_match_the_reference_on_cpu(pair, tag):
    from cream_amd.minivit_distill import distill_losses
    student, teacher = pair
    fix = fixture()
    x, _ = inputs("distill")
    student.zero_grad(set_to_none=True)
    total, parts = distill_losses(student, teacher, x, torch.zeros(2, dtype=torch.long), config(SETTINGS[tag]))
    total.backward()
    with torch.no_grad():
        assert max_rel(student(x), fix[f"{tag}|logits"]) <= TOL and max_rel(teacher(x), fix["teacher|logits"]) <= TOL
    errs = {}
    for k in ("soft", "attn", "hidden"):
        ref = float(fix[f"{tag}|loss|{k}"][0])
        errs["loss " + k] = abs(float(parts[k].detach()) - ref) / abs(ref)
    errs["loss total"] = abs(float(total.detach()) - float(fix[f"{tag}|loss|total"][0])) / float(fix[f"{tag}|loss|total"][0])
    assert float(parts["truth"]) == 0.0                                                    # alpha = 0
    grads = {k: p.grad for k, p in student.named_parameters() if p.grad is not None}
    no_grad = load_json("minivit_distill.json")["tap_shapes"][tag]["no_grad"]
    assert sorted(k for k, p in student.named_parameters() if p.grad is None) == no_grad
    errs.update(digest_errors(tag, grads))
    print(f"[minivit_distill cpu {tag}] worst {max(errs.values()):.2e}")
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    assert not bad, sorted(bad.items(), key=lambda t: -t[1])[:8]
    assert all(p.grad is None for p in teacher.parameters())


def _direct_relation(student, teacher, Ar):
    """The formula of the issue, window by window and group by group, in fp64."""
    total = 0.0
    for s, t in zip(student, teacher):
        B, N, Cs = s[0].shape
        Ct = t[0].shape[2]
        ds, dt = Cs // Ar, Ct // Ar
        layer = 0.0
        for i in range(3):
            for j in range(3):
                for b in range(B):
                    for g in range(Ar):
                        a_s = s[i][b, :, g * ds:(g + 1) * ds].double() @ s[j][b, :, g * ds:(g + 1) * ds].double().T / ds ** 0.5
                        a_t = t[i][b, :, g * dt:(g + 1) * dt].double() @ t[j][b, :, g * dt:(g + 1) * dt].double().T / dt ** 0.5
                        layer += float(-(torch.softmax(a_t, -1) * torch.log_softmax(a_s, -1)).sum())
        total += layer / (B * Ar * N)
    return total / (9 * len(student))


def test_relation_loss_takes_reference_tuples_and_qkv_taps_on_cpu():
    from cream_amd.minivit_distill import QkvTap, relation_loss
    g = torch.Generator().manual_seed(3)
    qkv_s = torch.randn(2, 196, 3 * 64, generator=g, requires_grad=True)
    qkv_t = torch.randn(2, 196, 3 * 96, generator=g)
    s_tap, t_tap = QkvTap(qkv_s, (14, 14, 7, 3)), QkvTap(qkv_t, (14, 14, 7, 3))
    s_tuple, t_tuple = s_tap.windows(), t_tap.windows()
    assert s_tuple[0].shape == (8, 49, 64) and t_tuple[2].shape == (8, 49, 96)
    # the tap's windows are the reference's roll + partition
    rolled = torch.roll(qkv_s.detach().view(2, 14, 14, 192), (-3, -3), (1, 2))
    assert torch.equal(s_tuple[1][5], rolled[1, 0:7, 7:14, 64:128].reshape(49, 64))
    single_s = tuple(torch.randn(3, 49, 128, generator=g) for _ in range(3))
    single_t = tuple(torch.randn(3, 49, 64, generator=g) for _ in range(3))
    for Ar in (1, 2):
        want = _direct_relation([s_tuple, single_s], [t_tuple, single_t], Ar)
        for s0, t0 in ((s_tuple, t_tuple), (s_tap, t_tap), (s_tap, t_tuple), (s_tuple, t_tap)):
            got = relation_loss([s0, single_s], [t0, single_t], Ar)
            assert abs(float(got) - want) / want <= TOL, (Ar, float(got), want)
    relation_loss([s_tap], [t_tuple], 2).backward()
    assert qkv_s.grad is not None and float(qkv_s.grad.abs().max()) > 0 and qkv_t.grad is None


def test_hidden_relation_loss_on_cpu_is_the_formula():
    from cream_amd.minivit_distill import hidden_loss, hidden_relation_loss
    g = torch.Generator().manual_seed(4)
    s = [torch.randn(2, 50, 24, generator=g), torch.randn(2, 13, 48, generator=g)]
    t = [torch.randn(2, 50, 40, generator=g), torch.randn(2, 13, 16, generator=g)]
    want = 0.0
    for a, b in zip(s, t):
        a, b = a.double(), b.double()
        a, b = a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)
        want += float(((a @ a.transpose(1, 2) - b @ b.transpose(1, 2)) ** 2).mean()) * 49 / 2
    assert abs(float(hidden_relation_loss(s, t)) - want) / want <= TOL
    assert abs(float(hidden_loss(s, s)) - 0.0) == 0.0 and float(hidden_loss([s[0]], [s[0] + 1.0])) == pytest.approx(1.0, rel=1e-6)


def test_usable_truth_tables(monkeypatch):
    from cream_amd import minivit_distill as D
    monkeypatch.delenv("CREAM_IRPE_FUSED", raising=False)
    bf, f32, dev = torch.bfloat16, torch.float32, "cuda:0"
    assert D.usable_relation(bf, bf, dev, 96, 128, 1, 7, 7, 8192, 8192)                  # the recipes' first tapped layer
    assert D.usable_relation(bf, bf, dev, 768, 1024, 1, 7, 7, 128, 128)                  # the last stage's widths
    assert D.usable_relation(bf, bf, dev, 128, 192, 2, 7, 7, 8, 8) and D.usable_relation(bf, bf, dev, 64, 64, 1, 8, 8, 4, 4)
    assert not D.usable_relation(f32, bf, dev, 96, 128, 1, 7, 7, 8, 8)                   # fp32 qkv
    assert not D.usable_relation(bf, f32, dev, 96, 128, 1, 7, 7, 8, 8)
    assert not D.usable_relation(bf, bf, "cpu", 96, 128, 1, 7, 7, 8, 8)
    assert not D.usable_relation(bf, bf, dev, 96, 128, 2, 7, 7, 8, 8)                    # C / Ar = 48
    assert not D.usable_relation(bf, bf, dev, 128, 96, 2, 7, 7, 8, 8)                    # ... on the teacher's side
    assert not D.usable_relation(bf, bf, dev, 96, 128, 1, 12, 12, 8, 8)                  # window 12: 144 tokens
    assert not D.usable_relation(bf, bf, dev, 96, 128, 1, 7, 7, 8, 2)                    # window counts differ
    assert not D.usable_relation(bf, bf, dev, 96, 128, 1, 7, None, 8, 8)                 # no square window
    assert not D.usable_relation(bf, bf, dev, 96, 128, 1, 7, 6, 8, 8)
    assert D.usable_hidden(f32, f32, dev) and D.usable_hidden(bf, f32, dev) and D.usable_hidden(f32, bf, dev)
    assert not D.usable_hidden(torch.float16, f32, dev) and not D.usable_hidden(f32, torch.float64, dev)
    assert not D.usable_hidden(f32, f32, "cpu")
    monkeypatch.setenv("CREAM_IRPE_FUSED", "0")
    assert not D.usable_relation(bf, bf, dev, 96, 128, 1, 7, 7, 8192, 8192) and not D.usable_hidden(f32, f32, dev)


def test_uncovered_taps_run_composed_without_touching_the_library(monkeypatch):
    """CPU tensors, fp32: `relation_loss` and `hidden_relation_loss` never load the library."""
    from cream_amd import _lib, minivit_distill as D
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    q = tuple(torch.randn(2, 49, 48) for _ in range(3))
    assert torch.isfinite(D.relation_loss([q], [q], 1)) and torch.isfinite(D.hidden_relation_loss([q[0]], [q[1]]))


def _relation_desc(**kw):
    from cream_amd import _lib
    d = _lib.RelationDesc()
    for side, C in ((d.s, 64), (d.t, 96)):
        side.q, side.k, side.v = 0x1000, 0x1000 + 2 * C, 0x1000 + 4 * C
        side.sb, side.sn, side.B, side.C, side.Hs, side.Ws, side.w, side.shift = 196 * 3 * C, 3 * C, 2, C, 14, 14, 7, 3
    d.Ar, d.want_grad, d.coef, d.part, d.part_blocks = 1, 0, 1.0, 0x9000, 1
    for k, v in kw.items():
        obj, name = (getattr(d, k[0]), k[2:]) if k[:2] in ("s_", "t_") else (d, k)
        setattr(obj, name, v)
    return d


def test_c_abi_argument_checks_return_codes_without_a_launch():
    from cream_amd import _lib
    lib = _lib.load()
    ok = lambda d: lib.cream_relation_loss_check(ctypes.byref(d))                          # noqa: E731
    assert ok(_relation_desc()) == 0 and lib.cream_relation_loss_check(None) == -1
    # the teacher as 8 partitioned windows against the student's two shifted 14 x 14 maps
    assert ok(_relation_desc(t_B=8, t_Hs=7, t_Ws=7, t_shift=0, t_sb=49 * 288)) == 0
    assert ok(_relation_desc(Ar=2, t_C=128, s_C=128, s_sn=384, s_sb=196 * 384, t_sn=384, t_sb=196 * 384)) == 0
    for bad in (dict(s_q=None), dict(t_v=None), dict(part=None), dict(part_blocks=0), dict(s_C=48), dict(Ar=2), dict(Ar=0),
                dict(s_w=9, s_Hs=18, s_Ws=18), dict(t_B=3), dict(t_Hs=7), dict(s_shift=7), dict(t_shift=-1), dict(s_sn=60),
                dict(s_sn=196), dict(s_k=0x1008), dict(t_w=0), dict(s_Hs=15), dict(want_grad=1),
                dict(want_grad=1, dq=0x2000, dk=0x3000, dv=0x4000, dsn=62, dsb=0)):
        d = _relation_desc(**bad)
        assert ok(d) == -1, bad
        assert lib.cream_relation_loss(ctypes.byref(d), None) == -1, bad                   # the same check, before any HIP call
    assert ok(_relation_desc(want_grad=1, dq=0x2000, dk=0x3000, dv=0x4000, dsn=192, dsb=196 * 192)) == 0
    assert lib.cream_relation_loss(ctypes.byref(_relation_desc(s_B=0, t_B=0)), None) == 0   # an empty batch launches nothing
    assert lib.cream_relation_loss_blocks(ctypes.byref(_relation_desc(s_B=0, t_B=0))) == 0
    h = _lib.HiddenRelationDesc()
    h.s, h.t, h.sn, h.tn, h.s_rinv, h.t_rinv, h.part = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    h.s_dtype, h.t_dtype, h.B, h.L, h.Cs, h.Ct, h.coef = _lib.F32, _lib.BF16, 2, 196, 64, 96, 1.0
    chk = lambda: lib.cream_hidden_relation_check(ctypes.byref(h))                         # noqa: E731
    assert chk() == 0
    h.want_grad = 1
    assert chk() == -1
    h.g, h.ds = 0x8000, 0x9000
    assert chk() == 0
    h.s_dtype = _lib.F16
    assert chk() == -2 and lib.cream_hidden_relation_loss(ctypes.byref(h), None) == -2
    h.s_dtype, h.L = _lib.F32, 0
    assert chk() == -1
    h.L, h.B = 196, 0
    assert lib.cream_hidden_relation_loss(ctypes.byref(h), None) == 0
    assert lib.cream_hidden_relation_padded(96) == 96 and lib.cream_hidden_relation_padded(100) == 128
    assert lib.cream_hidden_relation_parts(2, 196) == 8 and lib.cream_hidden_relation_parts(3, 49) == 3
