"""The distillation step of Mini-Swin — host-side mirror of MiniViT/Mini-Swin/main.py: `soft_cross_entropy` :33-37,
`cal_relation_loss` :39-57, `cal_hidden_loss` :59-64, `cal_hidden_relation_loss` :66-77 and the loss assembly of
`train_one_epoch_distill` :268-295 — on the kernels of csrc/distill_loss.hip.

The distilling models of cream_amd.miniswin hand out one TAP per listed layer where the reference hands out the tuple
(q, k, v) of partitioned windows:
  * `QkvTap` (fused attention path): the packed (B, Hs*Ws, 3C) projection of the unshifted map plus its geometry
    (Hs, Ws, w, shift) — the relation kernel reaches the shifted windows in the addressing, as the window attention does;
  * the reference's tuple of (B*nW, N, C) views (composed attention path).
`relation_loss` takes either kind on either side.

Two paths per layer:
  * fused — `usable_relation` / `usable_hidden` agree (a device, bf16 qkv, w*w <= 64, C/Ar a multiple of 32 on both sides,
    equal window counts; fp32 or bf16 hidden states): one launch returns the loss and, when the student requires grad, its
    gradient; backward multiplies the saved gradient by the incoming scalar.  Nothing of size N^2 per window or L^2 per image is
    written to memory;
  * composed — everything else (CPU, fp32 qkv, window 12, ...): the reference's arithmetic step by step.
`CREAM_IRPE_FUSED=0` switches the fused paths off together with the fused attentions.
"""
import ctypes
import math
import os
from dataclasses import dataclass, field
from typing import List

import torch
import torch.nn.functional as F

from . import _lib, timing

MAX_WINDOW_TOKENS = 64
DEPTH_MULTIPLE = 32


class QkvTap:
    """qkv (B, Hs*Ws, 3C) of the unshifted map, `geometry` = (Hs, Ws, w, shift) of the attention call that used it."""

    def __init__(self, qkv, geometry):
        self.qkv = qkv
        self.geometry = tuple(int(g) for g in geometry)

    def windows(self):
        """The reference's tuple: roll, partition -> three (B*nW, N, C) views of one tensor."""
        Hs, Ws, w, shift = self.geometry
        B, L, C3 = self.qkv.shape
        x = self.qkv.view(B, Hs, Ws, C3)
        if shift > 0:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        x = x.view(B, Hs // w, w, Ws // w, w, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, w * w, 3, C3 // 3)
        return x[:, :, 0], x[:, :, 1], x[:, :, 2]


def _fused_enabled():
    return os.environ.get("CREAM_IRPE_FUSED", "1") != "0"


def _describe(tap):
    """-> (dtype, device, C, w or None, windows) of a tap, from shapes alone."""
    if isinstance(tap, QkvTap):
        Hs, Ws, w, _ = tap.geometry
        return tap.qkv.dtype, tap.qkv.device, tap.qkv.shape[2] // 3, w, tap.qkv.shape[0] * (Hs // w) * (Ws // w)
    q = tap[0]
    w = math.isqrt(q.shape[1])
    return q.dtype, q.device, q.shape[2], (w if w * w == q.shape[1] else None), q.shape[0]


def usable_relation(s_dtype, t_dtype, device, Cs, Ct, Ar, w_s, w_t, windows_s, windows_t):
    """Decides from descriptors alone (no device is touched).  w_*: the window edge of a side, None when its token count is no
    square; windows_*: B * nW of a side."""
    if not _fused_enabled():
        return False
    if torch.device(device).type != "cuda" or s_dtype != torch.bfloat16 or t_dtype != torch.bfloat16:
        return False
    if w_s is None or w_s != w_t or w_s < 1 or w_s * w_s > MAX_WINDOW_TOKENS or windows_s != windows_t:
        return False
    if Ar < 1 or Cs % Ar or Ct % Ar or (Cs // Ar) % DEPTH_MULTIPLE or (Ct // Ar) % DEPTH_MULTIPLE:
        return False
    return True


def usable_hidden(s_dtype, t_dtype, device):
    if not _fused_enabled() or torch.device(device).type != "cuda":
        return False
    ok = (torch.float32, torch.bfloat16)
    return s_dtype in ok and t_dtype in ok


# ---- composed: the reference's arithmetic --------------------------------------------------------------------------------------
def soft_cross_entropy(predicts, targets):
    """:33-37."""
    student_likelihood = F.log_softmax(predicts, dim=-1)
    targets_prob = F.softmax(targets, dim=-1)
    return torch.sum(-targets_prob * student_likelihood, dim=-1).mean()


def _as_tuple(tap):
    return tap.windows() if isinstance(tap, QkvTap) else tap


def relation_loss_layer_composed(student, teacher, Ar):
    """One layer of :42-56 (the sum over the nine pairs, not yet divided)."""
    student, teacher = _as_tuple(student), _as_tuple(teacher)
    B, N, Cs = student[0].shape
    Ct = teacher[0].shape[2]
    loss = 0.
    for i in range(3):
        for j in range(3):
            mi = student[i].reshape(B, N, Ar, Cs // Ar).transpose(1, 2) / (Cs / Ar) ** 0.5
            mj = student[j].reshape(B, N, Ar, Cs // Ar).permute(0, 2, 3, 1)
            As = mi @ mj
            mi = teacher[i].reshape(B, N, Ar, Ct // Ar).transpose(1, 2) / (Ct / Ar) ** 0.5
            mj = teacher[j].reshape(B, N, Ar, Ct // Ar).permute(0, 2, 3, 1)
            loss = loss + soft_cross_entropy(As, mi @ mj)
    return loss


def hidden_relation_layer_composed(student_hidden, teacher_hidden):
    """One layer of :72-76."""
    s = F.normalize(student_hidden, dim=-1)
    t = F.normalize(teacher_hidden, dim=-1)
    return torch.mean((s @ s.transpose(-1, -2) - t @ t.transpose(-1, -2)) ** 2) * 49


def hidden_loss(student_hidden_list, teacher_hidden_list):
    """:59-64."""
    loss = 0.
    for s, t in zip(student_hidden_list, teacher_hidden_list):
        loss = loss + F.mse_loss(s, t)
    return loss / len(student_hidden_list)


# ---- fused relation loss -------------------------------------------------------------------------------------------------------
def _views_ok(views):
    q = views[0]
    es = q.element_size()
    return all(v.dim() == 3 and v.stride() == q.stride() and v.stride(2) == 1 and v.stride(0) % 8 == 0 and v.stride(1) % 8 == 0
               and v.data_ptr() % 16 == 0 and v.dtype == q.dtype for v in views) and es == 2


def _side(tap):
    """-> ((q, k, v) views (maps, tokens, C) with equal strides and unit channel stride, (maps, Hs, Ws, w, shift))."""
    if isinstance(tap, QkvTap):
        Hs, Ws, w, shift = tap.geometry
        qkv = tap.qkv if tap.qkv.stride(2) == 1 else tap.qkv.contiguous()
        B, L, C3 = qkv.shape
        v = qkv.view(B, L, 3, C3 // 3)
        views = (v[:, :, 0], v[:, :, 1], v[:, :, 2])
        geom = (B, Hs, Ws, w, shift)
    else:
        views = tuple(tap)
        w = math.isqrt(views[0].shape[1])
        geom = (views[0].shape[0], w, w, w, 0)
    if not _views_ok(views):
        packed = torch.stack([v.detach() for v in views], dim=2)        # (maps, tokens, 3, C), contiguous
        views = (packed[:, :, 0], packed[:, :, 1], packed[:, :, 2])
    return views, geom


def _fill_side(d, views, geom):
    d.q, d.k, d.v = (v.data_ptr() for v in views)
    d.sb, d.sn = views[0].stride(0), views[0].stride(1)
    d.B, d.Hs, d.Ws, d.w, d.shift = geom
    d.C = views[0].shape[2]


def _relation_flops(items, N, ds, dt, grad):
    NP = 64
    return items * (9 * 2.0 * NP * NP * (ds + dt) + (6 * 2.0 * NP * 3 * NP * ds if grad else 0.0))


def relation_core(s_views, s_geom, t_views, t_geom, Ar, coef, dviews=None):
    """One launch.  *_views: (q, k, v) bf16 views (maps, tokens, C); *_geom = (maps, Hs, Ws, w, shift); dviews: where the
    gradient with respect to the student's q, k, v goes (None: forward only).  -> the loss (0-dim fp32).  Outside autograd."""
    d = _lib.RelationDesc()
    _fill_side(d.s, s_views, s_geom)
    _fill_side(d.t, t_views, t_geom)
    d.Ar, d.want_grad, d.coef = Ar, int(dviews is not None), coef
    dev = s_views[0].device
    lib = _lib.load()
    with torch.cuda.device(dev):
        blocks = lib.cream_relation_loss_blocks(ctypes.byref(d))
        if blocks < 0:
            _lib.check(blocks, "cream_relation_loss_blocks")
        part = torch.zeros(max(blocks, 1), dtype=torch.float32, device=dev)
        d.part, d.part_blocks = part.data_ptr(), max(blocks, 1)
        if dviews is not None:
            d.dq, d.dk, d.dv = (v.data_ptr() for v in dviews)
            d.dsb, d.dsn = dviews[0].stride(0), dviews[0].stride(1)
        w = s_geom[3]
        items = s_geom[0] * (s_geom[1] // w) * (s_geom[2] // w) * Ar
        with timing.region("relation_loss", flops=_relation_flops(items, w * w, d.s.C // Ar, d.t.C // Ar, dviews is not None)):
            rc = lib.cream_relation_loss(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "cream_relation_loss")
    return part.sum()                                   # fixed order over the persistent grid


class _RelationMap(torch.autograd.Function):
    """Student = a QkvTap's packed projection: one gradient tensor in the same layout."""

    @staticmethod
    def forward(ctx, qkv, geometry, t_views, t_geom, Ar, coef):
        B, L, C3 = qkv.shape
        s_views, s_geom = _side(QkvTap(qkv, geometry))
        dviews = None
        if ctx.needs_input_grad[0]:
            dqkv = torch.empty((B, L, 3, C3 // 3), dtype=qkv.dtype, device=qkv.device)
            dviews = (dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2])
            ctx.save_for_backward(dqkv.view(B, L, C3))
        return relation_core(s_views, s_geom, t_views, t_geom, Ar, coef, dviews)

    @staticmethod
    def backward(ctx, gout):
        (dqkv,) = ctx.saved_tensors
        return (dqkv * gout.to(dqkv.dtype),) + (None,) * 5


class _RelationTuple(torch.autograd.Function):
    """Student = the reference's tuple of windowed (B*nW, N, C) tensors."""

    @staticmethod
    def forward(ctx, q, k, v, t_views, t_geom, Ar, coef):
        s_views, s_geom = _side((q, k, v))
        dviews = None
        if any(ctx.needs_input_grad[:3]):
            B_, N, C = q.shape
            dqkv = torch.empty((B_, N, 3, C), dtype=q.dtype, device=q.device)
            dviews = (dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2])
            ctx.save_for_backward(dqkv)
        return relation_core(s_views, s_geom, t_views, t_geom, Ar, coef, dviews)

    @staticmethod
    def backward(ctx, gout):
        (dqkv,) = ctx.saved_tensors
        g = dqkv * gout.to(dqkv.dtype)
        return (g[:, :, 0], g[:, :, 1], g[:, :, 2]) + (None,) * 4


def relation_loss(student_taps, teacher_taps, Ar=1):
    """`cal_relation_loss` (:39-57) over lists of taps (QkvTap or the reference's (q, k, v) tuples, freely mixed)."""
    layers = len(student_taps)
    total = 0.
    for s, t in zip(student_taps, teacher_taps):
        sd, dev, Cs, ws, nws = _describe(s)
        td, _, Ct, wt, nwt = _describe(t)
        if usable_relation(sd, td, dev, Cs, Ct, Ar, ws, wt, nws, nwt):
            with torch.no_grad():
                t_views, t_geom = _side(t if isinstance(t, QkvTap) else tuple(x.detach() for x in t))
            coef = 1.0 / (float(nws) * Ar * ws * ws * 9.0 * layers)
            if isinstance(s, QkvTap):
                total = total + _RelationMap.apply(s.qkv, s.geometry, t_views, t_geom, Ar, coef)
            else:
                total = total + _RelationTuple.apply(s[0], s[1], s[2], t_views, t_geom, Ar, coef)
        else:
            total = total + relation_loss_layer_composed(s, t, Ar) / (9. * layers)
    return total


# ---- fused hidden relation loss -------------------------------------------------------------------------------------------------
def hidden_core(s, t, coef, want_grad):
    """s (B, L, Cs), t (B, L, Ct) contiguous, fp32 or bf16 -> (loss (0-dim fp32), ds in s's dtype or None).  Outside autograd."""
    B, L, Cs = s.shape
    Ct = t.shape[2]
    dev = s.device
    lib = _lib.load()
    code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}
    csp, ctp = lib.cream_hidden_relation_padded(Cs), lib.cream_hidden_relation_padded(Ct)
    d = _lib.HiddenRelationDesc()
    sn = torch.empty((B, L, csp), dtype=torch.bfloat16, device=dev)
    tn = torch.empty((B, L, ctp), dtype=torch.bfloat16, device=dev)
    rinv = torch.empty((2, B, L), dtype=torch.float32, device=dev)
    part = torch.zeros(max(lib.cream_hidden_relation_parts(B, L), 1), dtype=torch.float32, device=dev)
    g = torch.empty((B, L, csp), dtype=torch.float32, device=dev) if want_grad else None
    ds = torch.empty_like(s) if want_grad else None
    d.s, d.t, d.s_dtype, d.t_dtype = s.data_ptr(), t.data_ptr(), code[s.dtype], code[t.dtype]
    d.B, d.L, d.Cs, d.Ct, d.want_grad, d.coef = B, L, Cs, Ct, int(want_grad), coef
    d.sn, d.tn, d.s_rinv, d.t_rinv, d.part = sn.data_ptr(), tn.data_ptr(), rinv[0].data_ptr(), rinv[1].data_ptr(), part.data_ptr()
    if want_grad:
        d.g, d.ds = g.data_ptr(), ds.data_ptr()
    tiles = (L + 63) // 64
    flops = B * tiles * tiles * 2.0 * 64 * 64 * ((csp + ctp) * (((csp + 127) // 128) if want_grad else 1) + (csp if want_grad else 0))
    with torch.cuda.device(dev), timing.region("hidden_relation_loss", flops=flops):
        rc = lib.cream_hidden_relation_loss(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_hidden_relation_loss")
    return part.sum(), ds


class _HiddenRelation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t, coef):
        loss, ds = hidden_core(s.contiguous(), t.detach().contiguous(), coef, ctx.needs_input_grad[0])
        if ds is not None:
            ctx.save_for_backward(ds)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (ds,) = ctx.saved_tensors
        return ds * gout.to(ds.dtype), None, None


def hidden_relation_loss(student_hidden, teacher_hidden):
    """`cal_hidden_relation_loss` (:66-77) over lists of (B, L, C) hidden states."""
    layers = len(student_hidden)
    total = 0.
    for s, t in zip(student_hidden, teacher_hidden):
        if s.dim() == 3 and usable_hidden(s.dtype, t.dtype, s.device):
            B, L, _ = s.shape
            total = total + _HiddenRelation.apply(s, t, 49.0 / (float(B) * L * L * layers))
        else:
            total = total + hidden_relation_layer_composed(s, t) / layers
    return total


# ---- the step -----------------------------------------------------------------------------------------------------------------
@dataclass
class DistillConfig:
    """DISTILL.* of Mini-Swin/config.py with the reference's defaults; the published recipes pass attn_loss, hidden_loss,
    hidden_relation, alpha 0 and hidden_weight 0.1."""
    student_layers: List[int] = field(default_factory=list)
    teacher_layers: List[int] = field(default_factory=list)
    alpha: float = 0.0
    temperature: float = 1.0
    ar: int = 1
    qkv_weight: float = 1.0
    hidden_weight: float = 1.0
    attn_loss: bool = True
    hidden_loss: bool = True
    hidden_relation: bool = True


def truth_loss(outputs, targets):
    """Hard labels: cross entropy; soft (mixup) targets: timm's SoftTargetCrossEntropy."""
    if targets.dtype in (torch.int64, torch.int32):
        return F.cross_entropy(outputs, targets.long())
    return torch.sum(-targets * F.log_softmax(outputs, dim=-1), dim=-1).mean()


def distill_losses(student, teacher, samples, targets, cfg):
    """The body of `train_one_epoch_distill` (:268-295): -> (total, dict(truth, soft, attn, hidden))."""
    out = student(samples, cfg.student_layers, is_attn_loss=cfg.attn_loss, is_hidden_loss=cfg.hidden_loss,
                  is_hidden_org=cfg.hidden_relation)
    tapped = cfg.attn_loss or cfg.hidden_loss
    outputs = out[0] if tapped else out
    qkv_s = out[1] if cfg.attn_loss else None
    hidden_s = out[-1] if cfg.hidden_loss else None
    with torch.no_grad():
        if tapped:
            outputs_t, qkv_t, hidden_t = teacher(samples, cfg.teacher_layers, is_attn_loss=True, is_hidden_loss=True)
        else:
            outputs_t = teacher(samples)
    outputs, outputs_t = outputs.float(), outputs_t.float()
    parts = dict(truth=cfg.alpha * truth_loss(outputs, targets),
                 soft=(1.0 - cfg.alpha) * soft_cross_entropy(outputs / cfg.temperature, outputs_t / cfg.temperature))
    zero = torch.zeros((), device=outputs.device)
    parts["attn"] = cfg.qkv_weight * relation_loss(qkv_s, qkv_t, cfg.ar) if cfg.attn_loss else zero
    if cfg.hidden_loss:
        criterion = hidden_relation_loss if cfg.hidden_relation else hidden_loss
        parts["hidden"] = cfg.hidden_weight * criterion(hidden_s, hidden_t)
    else:
        parts["hidden"] = zero
    return parts["truth"] + parts["soft"] + parts["attn"] + parts["hidden"], parts
