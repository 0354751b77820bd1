"""Mini-Swin at window 12 on the GPU, block level through `SwinTransformerBlock.forward_feature` under bf16 autocast:
A. head-mixing blocks of the shapes in `window_attn_mix_large.ACCEPTED` take csrc/window_attn_mix_large.hip (both repeats, the
   shift alternating), plain blocks of `PLAIN_ACCEPTED` csrc/window_attn_large.hip, and no composed softmax runs;
B. accuracy by the rule of test_window_attn_gpu.py::test_fused_against_composed: err(fused) <= max(2 err(composed bf16), 2^-7)
   for every tensor, both against the fp32 composed branch; d proj_l.bias (zero in exact arithmetic) absolutely;
C. one distillation step of a tiny 384-style pair (window 12, two stages): the taps of both routes go through `relation_loss`;
D. reruns are bit-identical.
The shapes are put into the accepted sets here (what the default sets hold is decided by measurement, not by these tests)."""
import pytest
import torch

from helpers import max_rel
from test_window_attn_gpu import fused_off

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIX = {"window_attn_mix_large_fwd", "window_attn_mix_large_bwd"}
PLAIN = {"window_attn_large_fwd", "window_attn_large_bwd"}
SMALL = {"window_attn_fwd", "window_attn_bwd"}


@pytest.fixture(autouse=True)
def accepted(monkeypatch):
    from cream_amd import window_attn_mix_large as W
    shapes = frozenset({(12, 24, 24, 16), (12, 24, 36, 4), (12, 24, 24, 2), (12, 12, 12, 4)})
    monkeypatch.setattr(W, "ACCEPTED", shapes)
    monkeypatch.setattr(W, "PLAIN_ACCEPTED", shapes)
    monkeypatch.setattr(W, "EXCLUDED", frozenset())
    monkeypatch.setattr(W, "PLAIN_EXCLUDED", frozenset())


class Repeats(torch.nn.Module):
    """The attention halves of a shared block's repeats — norm1, qkv, window attention, proj — through the block's own code:
    repeat r is shifted for odd r (a shared block) or as `shifts` says."""

    def __init__(self, H, res, mix, repeats, shifts=None, seed=0):
        super().__init__()
        from cream_amd import miniswin
        torch.manual_seed(seed)
        self.shifts = shifts if shifts is not None else [r % 2 == 1 for r in range(repeats)]
        self.blk = miniswin.SwinTransformerBlock(H * 32, res, H, window_size=12, shift_size=6, drop_path=[0.] * repeats,
                                                 is_sep_layernorm=mix, is_transform_heads=mix)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for n, p in self.blk.named_parameters():
                if 'relative_position_bias_table' in n:
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
                elif n.startswith('proj_l') or n.startswith('proj_w'):
                    p.copy_(torch.eye(H) + 0.3 * torch.randn(H, H, generator=g) if p.dim() == 2 else 0.2 * torch.randn(H, generator=g))
                elif n == 'attn.qkv.bias':
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
                elif n.startswith('norm1_list') and n.endswith('weight'):
                    p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
        self.blk.mlp = torch.nn.Identity()                    # the attention half alone
        if mix:
            self.blk.norm2_list = torch.nn.ModuleList([torch.nn.Identity() for _ in range(repeats)])
        else:
            self.blk.norm2 = torch.nn.Identity()

    def forward(self, x):
        for r, s in enumerate(self.shifts):
            x = self.blk.forward_feature(x, is_shift=s, layer_index=r) * 0.5          # 0.5 (x + attn + x + attn): keeps the scale
        return x


def tensors_of(m):
    b = m.blk
    out = {"d qkv.weight": b.attn.qkv.weight.grad, "d table": b.attn.relative_position_bias_table.grad}
    if b.proj_l is not None:
        for r in range(len(b.proj_l)):
            out.update({f"d proj_l.{r}.weight": b.proj_l[r].weight.grad, f"d proj_w.{r}.weight": b.proj_w[r].weight.grad,
                        f"d proj_w.{r}.bias": b.proj_w[r].bias.grad, f"d proj_l.{r}.bias": b.proj_l[r].bias.grad})
    return out


def run(m, x, gy, autocast, fused):
    """-> ({name: tensor}, regions seen, composed softmax calls)"""
    from cream_amd import timing
    m.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    calls = []
    hook = m.blk.attn.softmax.register_forward_hook(lambda *a: calls.append(1))
    timing.reset()
    timing.enable(True)
    try:
        if fused:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = m(x)
        else:
            with fused_off(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = m(x)
        (y.float() * gy).sum().backward()
    finally:
        timing.enable(False)
        hook.remove()
    res = {"out": y.detach().float().cpu(), "dx": x.grad.detach().float().cpu()}
    res.update({k: v.detach().float().cpu() for k, v in tensors_of(m).items()})
    return res, set(timing.summary()), len(calls)


def inputs(B, res, H, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, res[0] * res[1], H * 32, generator=g).bfloat16().float().to(DEV)
    gy = torch.randn(B, res[0] * res[1], H * 32, generator=g).to(DEV)
    return x, gy


def check_rule(tag, ref, comp, fus):
    bad = []
    for k in ref:
        if "proj_l" in k and k.endswith("bias"):
            eb, ec = float(comp[k].abs().max()), float(fus[k].abs().max())
            bound = max(2 * eb, 2.0 ** -7 * float(ref[k.replace("bias", "weight")].abs().max()))
        else:
            eb, ec = max_rel(comp[k], ref[k]), max_rel(fus[k], ref[k])
            bound = max(2 * eb, 2.0 ** -7)
        print(f"[miniswin 384 {tag}] {k:18s} composed bf16 {eb:.3e}  fused {ec:.3e}  bound {bound:.3e}")
        if not ec <= bound:
            bad.append((k, eb, ec, bound))
    return bad


CASES = {
    "stage3": dict(H=16, res=(24, 24), B=1),                  # the recipe's stage-3 shape, both repeats
    "small": dict(H=4, res=(24, 36), B=2),                    # a non-square map, six windows per image
}
_RESULTS = {}


def results(tag, mix=True):
    key = (tag, mix)
    if key not in _RESULTS:
        c = CASES[tag]
        m = Repeats(c["H"], c["res"], mix, 2, shifts=None if mix else [False, True]).to(DEV)
        if not mix:
            assert m.blk.attn_mask is not None                # a plain shared pair: the mask in both repeats, as the block does
        x, gy = inputs(c["B"], c["res"], c["H"])
        ref = run(m, x, gy, autocast=False, fused=True)       # fp32: the module itself stays composed
        comp = run(m, x, gy, autocast=True, fused=False)
        fus = run(m, x, gy, autocast=True, fused=True)
        again = run(m, x, gy, autocast=True, fused=True)
        _RESULTS[key] = (ref, comp, fus, again)
    return _RESULTS[key]


@pytest.mark.parametrize("tag", list(CASES))
def test_mixed_blocks_take_the_new_kernels(tag):
    (ref, na, ca), (comp, nb, cb), (fus, nc, cc), _ = results(tag)
    assert not (MIX | PLAIN | SMALL) & na and not (MIX | PLAIN | SMALL) & nb, (na, nb)
    assert ca == 2 and cb == 2, (ca, cb)                      # the composed softmax of both repeats
    assert MIX <= nc and not (PLAIN | SMALL) & nc and cc == 0, (nc, cc)
    assert not check_rule(tag, ref, comp, fus)


def test_plain_block_takes_the_large_kernels():
    (ref, na, ca), (comp, nb, cb), (fus, nc, cc), _ = results("small", mix=False)
    assert not (MIX | PLAIN | SMALL) & na and not (MIX | PLAIN | SMALL) & nb and ca == 2 and cb == 2, (na, nb, ca, cb)
    assert PLAIN <= nc and not (MIX | SMALL) & nc and cc == 0, (nc, cc)
    assert not check_rule("plain", ref, comp, fus)


@pytest.mark.parametrize("tag,mix", [("stage3", True), ("small", True), ("small", False)])
def test_reruns_are_bit_identical(tag, mix):
    _, _, (a, _, _), (b, _, _) = results(tag, mix)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_unlisted_shape_stays_composed(monkeypatch):
    from cream_amd import window_attn_mix_large as W
    monkeypatch.setattr(W, "ACCEPTED", frozenset())
    monkeypatch.setattr(W, "PLAIN_ACCEPTED", frozenset())
    c = CASES["small"]
    for mix in (True, False):
        m = Repeats(c["H"], c["res"], mix, 1).to(DEV)
        x, gy = inputs(1, c["res"], c["H"])
        _, names, calls = run(m, x, gy, autocast=True, fused=True)
        assert not (MIX | PLAIN | SMALL) & names and calls == 1, (mix, names, calls)


# ---- C. one distillation step ---------------------------------------------------------------------------------------------------
MODEL = dict(img_size=96, patch_size=4, num_classes=10, embed_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=12,
             drop_path_rate=0.0)                               # maps 24 x 24 (four windows, shifted) and 12 x 12 (one window)
LAYERS = [1, 3]
WEIGHTS = ("layers.0.blocks.0.attn.qkv.weight", "layers.0.blocks.0.attn.relative_position_bias_table",
           "layers.0.blocks.0.proj_l.1.weight", "layers.1.blocks.0.proj_w.0.weight", "layers.1.blocks.0.attn.qkv.weight")
_PAIR = {}


def pair():
    if not _PAIR:
        from cream_amd import miniswin
        torch.manual_seed(3)
        student = miniswin.SwinTransformerMiniViTDistill(**MODEL, separate_layer_num_list=[1, 1], is_sep_layernorm=True,
                                                         is_transform_FFN=True, is_transform_heads=True, is_student=True, fit_size_C=64)
        teacher = miniswin.SwinTransformerDistill(**MODEL)
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for model in (student, teacher):
                for n, p in model.named_parameters():
                    if 'relative_position_bias_table' in n:
                        p.copy_(0.3 * torch.randn(p.shape, generator=g))
                    elif '.proj_l.' in n or '.proj_w.' in n:
                        H = p.shape[0]
                        p.copy_(torch.eye(H) + 0.3 * torch.randn(H, H, generator=g) if p.dim() == 2 else 0.2 * torch.randn(H, generator=g))
        _PAIR["models"] = (student.eval().to(DEV), teacher.eval().to(DEV))
    return _PAIR["models"]


def run_step(autocast, fused):
    from cream_amd import timing
    from cream_amd.minivit_distill import DistillConfig, distill_losses
    student, teacher = pair()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 96, 96, generator=g).to(DEV)
    y = torch.zeros(2, dtype=torch.long, device=DEV)
    cfg = DistillConfig(student_layers=LAYERS, teacher_layers=LAYERS, hidden_relation=True)
    student.zero_grad(set_to_none=True)
    taps = []
    from cream_amd import minivit_distill as D
    real = D.relation_loss
    D.relation_loss = lambda s, t, ar=1: (taps.append((list(s), list(t))), real(s, t, ar))[1]
    timing.reset()
    timing.enable(True)
    try:
        if fused:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                total, parts = distill_losses(student, teacher, x, y, cfg)
        else:
            with fused_off(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                total, parts = distill_losses(student, teacher, x, y, cfg)
        total.backward()
    finally:
        timing.enable(False)
        D.relation_loss = real
    out = {"total": total.detach().float().cpu().reshape(1), "attn": parts["attn"].detach().float().cpu().reshape(1)}
    params = dict(student.named_parameters())
    out.update({"d " + n: params[n].grad.detach().float().cpu() for n in WEIGHTS})
    return out, set(timing.summary()), taps


def test_distillation_step_through_both_routes():
    from cream_amd.minivit_distill import QkvTap
    ref, na, _ = run_step(autocast=False, fused=True)
    comp, nb, tb = run_step(autocast=True, fused=False)
    fus, nc, tc = run_step(autocast=True, fused=True)
    again, _, _ = run_step(autocast=True, fused=True)
    assert not (MIX | PLAIN) & na and not (MIX | PLAIN) & nb, (na, nb)
    assert MIX | {"window_attn_large_fwd"} <= nc, nc                               # the teacher runs without grad: no backward
    (s_taps, t_taps), = tc
    assert len(s_taps) == len(t_taps) == 2
    assert all(isinstance(t, QkvTap) for t in s_taps + t_taps)                     # both new routes hand their map to the loss
    assert [t.geometry for t in s_taps] == [(24, 24, 12, 6), (12, 12, 12, 0)] == [t.geometry for t in t_taps]
    assert not any(isinstance(t, QkvTap) for t in tb[0][0] + tb[0][1])             # the all-composed step: the reference's tuples
    bad = []
    for k in ref:
        eb, ec = max_rel(comp[k], ref[k]), max_rel(fus[k], ref[k])
        bound = max(2 * eb, 2.0 ** -7)
        print(f"[miniswin 384 distill step] {k:60s} composed bf16 {eb:.3e}  fused {ec:.3e}  bound {bound:.3e}")
        if not ec <= bound:
            bad.append((k, eb, ec, bound))
    assert not bad, bad
    for k in fus:
        assert torch.equal(fus[k], again[k]), k
