"""One affinity-mimicking distillation step of TinyCLIP — the body of `train_one_epoch`
(TinyCLIP/src/training/train.py:84-560) for the dense student / frozen teacher recipe of the shipped scripts
(`--distillation --local-loss --gather-with-grad --logit-scale 50 --norm_gradient_clip 5`, script/*.sh):

    teacher (no grad, autocast): normalised image / text features, logit scale fixed to `logit_scale`     (:405-420)
    student (autocast):          normalised features, exp(logit scale)                                   (:227-242)
    loss = 0.5 w (soft CE image->text) + 0.5 w (soft CE text->image),  w = alpha * distillation weight   (:173-186)
           [+ (1 - alpha) * weight * the hard CLIP loss when alpha < 1]                                   (:192-195)
    backward; clip the global gradient norm; optimizer step                                              (:505-513)
    student logit scale: filled with ln(logit_scale) when that flag is given, else clamped to [0, ln 100] (:526-530)

bf16 autocast needs no loss scaler (the reference's `amp` = fp16 + GradScaler; `amp_bfloat16` is its own bf16 mode,
precision.py:7-11).  Multi-GPU: one process per GPU; the only exchanges are the feature gathers inside `ClipSoftLoss`
(cream_amd/tinyclip/soft_loss.py) and the gradient average of `GradReducer`.

Mask learning (automatic weight inheritance; all of it inactive while no tower has an `l0_module`): the Lagrangian sparsity
term — joint over both towers with `total_loss_flag`, per tower otherwise (:256-312) —, a second optimizer for the l0
parameters (optimizer.py:72-99: `make_l0_optimizer`), `constrain_parameters()` after the step (:509-520), and `fuse_masks`
(:333-362) for the prune step.  Single process only.
"""
import math

import torch
import torch.nn.functional as F

from .. import grad_clip
from .soft_loss import ClipSoftLoss, gather_features_with_grad


def hard_clip_loss(image_features, text_features, logit_scale, rank=0, group=None):
    """open_clip/loss.py `ClipLoss` with local_loss + gather_with_grad: contrastive CE against the global batch."""
    all_image, all_text = gather_features_with_grad(image_features, text_features, True, group)
    li = logit_scale * image_features @ all_text.T
    lt = logit_scale * text_features @ all_image.T
    n = image_features.shape[0]
    labels = torch.arange(n, device=li.device) + n * rank
    return (F.cross_entropy(li, labels) + F.cross_entropy(lt, labels)) / 2


def tower_bucket_of(name, blocks_per_bucket=4):
    """Bucket key of a student parameter: the reference wraps the image tower, the text tower and the logit scale in three
    separate DDP instances (`ddpify`, open_clip/model.py:977-988), so each tower's gradients travel as soon as THAT tower's
    backward has produced them.  Here: one GradReducer whose buckets never cross a tower — `<tower>.tr<k>` for every
    `blocks_per_bucket` consecutive transformer blocks (a ViT-39M/16 block is ~7 MB of fp32 gradients: 4 per message keeps
    the xGMI links busy without waiting for the whole tower), `<tower>.rest` for embeddings / projections / final norm."""
    parts = name.split(".")
    tower = parts[0]
    if "resblocks" in parts:
        return f"{tower}.tr{int(parts[parts.index('resblocks') + 1]) // blocks_per_bucket:02d}"
    return tower if tower == "_logit_scale" else f"{tower}.rest"


def make_reducer(student, group=None, mode="allreduce", blocks_per_bucket=4):
    """`ddpify` of the step (model.py:977-988): per-tower gradient buckets on the side-stream reducer (cream_amd/comm.py).  No
    active-slice packing: TinyCLIP's towers are dense."""
    from ..comm import GradReducer
    return GradReducer(student, process_group=group, mode=mode, slice_of=None,
                       bucket_of=lambda n: tower_bucket_of(n, blocks_per_bucket))


def l0_modules(student):
    """-> (image tower's l0_module or None, text tower's)."""
    return getattr(student._image_encoder, "l0_module", None), getattr(student._text_encoder, "l0_module", None)


def student_parameters(student):
    """The parameters of the student's own optimizer: everything but the l0 modules' (optimizer.py:46-48)."""
    return [p for n, p in student.named_parameters() if p.requires_grad and "l0_module" not in n]


def make_l0_optimizer(student, l0lr=-0.02, lr_l0=0.02):
    """optimizer.py:72-99: AdamW without weight decay, the log-alphas at `lr_l0`, the two Lagrange multipliers at `l0lr` —
    negative: gradient ASCENT on them.  (A negative rate is given to the optimizer as its magnitude with `maximize`, which
    is the same update when the weight decay is 0.)"""
    groups = []
    for enc in (student._image_encoder, student._text_encoder):
        if getattr(enc, "l0_module", None) is None:
            continue
        named = [(n, p) for n, p in enc.l0_module.named_parameters() if p.requires_grad]
        for params, lr in (([p for n, p in named if "lambda" not in n], lr_l0), ([p for n, p in named if "lambda" in n], l0lr)):
            groups.append(dict(params=params, weight_decay=0.0, lr=abs(lr), maximize=lr < 0))
    return torch.optim.AdamW(groups)


def fuse_masks(student, image=None, text=None):
    """train.py:333-362: one eval forward per tower (it leaves the deterministic masks on the modules), `prune()`, `l0_module =
    None`.  `image` / `text`: any valid input of the towers (default: the reference's random image and token ids).  The caller
    rebuilds its optimizers: the pruned towers have new parameters."""
    ie, te = student._image_encoder, student._text_encoder
    dev = next(student.parameters()).device
    with torch.no_grad():
        if getattr(ie, "l0_module", None) is not None:
            ie.eval()
            size = ie.visual.image_size
            ie(image if image is not None else torch.randn((1, 3) + tuple(size), device=dev))
            student._image_encoder = ie.prune()
            student._image_encoder.l0_module = None
        if getattr(te, "l0_module", None) is not None:
            te.eval()
            te(text if text is not None else torch.randint(0, min(100, te.vocab_size), (1, te.context_length), device=dev))
            student._text_encoder = te.prune()
            student._text_encoder.l0_module = None
    return student


class DistillStep:
    def __init__(self, student, teacher, optimizer, *, logit_scale=50.0, distillation_alpha=1.0, distillation_weight=1.0,
                 norm_gradient_clip=5.0, amp_dtype=torch.bfloat16, rank=0, world_size=1, group=None, reducer=None,
                 l0_optimizer=None, total_loss_flag=False, start_step=0):
        if reducer is not None and any(m is not None for m in l0_modules(student)):
            raise NotImplementedError("DistillStep: a gradient reducer together with an l0_module — multi-rank mask learning is "
                                      "not supported (the reducer's buckets do not hold the l0 parameters)")
        self.l0_optimizer, self.total_loss_flag, self.step_index, self.last_sparsity = l0_optimizer, total_loss_flag, start_step, None
        self.student, self.teacher, self.optimizer = student, teacher, optimizer
        self.logit_scale, self.alpha, self.weight, self.clip = logit_scale, distillation_alpha, distillation_weight, norm_gradient_clip
        self.amp_dtype, self.rank, self.group, self.reducer = amp_dtype, rank, group, reducer
        self.soft_loss = ClipSoftLoss(local_loss=True, gather_with_grad=True, rank=rank, world_size=world_size, group=group)
        for p in teacher.parameters():
            p.requires_grad = False
        teacher.eval()
        self.params = student_parameters(student)     # (the clipped ones: the l0 parameters are not, train.py:505-513)
        self.last_grad_norm = None

    def _autocast(self, device):
        on = self.amp_dtype != torch.float32 and device.type == "cuda"
        return torch.autocast("cuda", dtype=self.amp_dtype if on else torch.bfloat16, enabled=on)

    def teacher_outputs(self, images, texts):
        with torch.no_grad(), self._autocast(images.device):
            if self.logit_scale is not None:
                self.teacher.logit_scale.fill_(math.log(self.logit_scale))                 # train.py:408-409
            ti = F.normalize(self.teacher.encode_image(images), dim=-1)
            tt = F.normalize(self.teacher.encode_text(texts), dim=-1)
            return ti, tt, self.teacher.logit_scale.exp()

    def loss(self, images, texts):
        ti, tt, ts = self.teacher_outputs(images, texts)
        with self._autocast(images.device):
            fi, ft, s = self.student(images, texts, normalized=True)
            total = 0.0
            if self.alpha > 0.0 and self.weight > 0.0:
                i2t, t2i = self.soft_loss(fi, ft, s, ti, tt, ts, average_two_losses=False)
                total = total + 0.5 * self.alpha * self.weight * (i2t + t2i)
            if self.alpha < 1.0 and self.weight > 0.0:
                total = total + (1.0 - self.alpha) * self.weight * hard_clip_loss(fi, ft, s, self.rank, self.group)
            total = total + self.lagrangian_loss()
        return total

    def lagrangian_loss(self):
        """train.py:256-312 at `self.step_index`; 0.0 without an l0_module.  Leaves expected / target sparsity in `last_sparsity`."""
        img, txt = l0_modules(self.student)
        if img is None and txt is None:
            return 0.0
        step = self.step_index
        if self.total_loss_flag and img is not None and txt is not None:
            remain = txt.get_num_parameters_and_constraint("hidden" in txt.types) + img.get_num_parameters_and_constraint("hidden" in img.types)
            expected = 1 - remain / (txt.prunable_model_size + img.prunable_model_size)
            target = sum(m.get_target_sparsity(step) if m.lagrangian_warmup > 0 else m.target_sparsity for m in (img, txt)) / 2
            gap = torch.maximum(target - expected, torch.tensor(0.0, device=expected.device))
            self.last_sparsity = dict(expected=float(expected.detach()), target=target)
            return (img.lambda_1 + txt.lambda_1) / 2 * gap + (img.lambda_2 + txt.lambda_2) / 2 * gap.square()
        total, self.last_sparsity = 0.0, {}
        for name, m in (("image", img), ("text", txt)):
            if m is not None:
                loss, expected, target = m.lagrangian_regularization(step)
                total = total + loss
                self.last_sparsity[name] = dict(expected=expected, target=target)
        return total

    def step(self, images, texts):
        if self.reducer is not None:
            # the reducer owns the gradients (views into its flat arena): zero-fill them in place and arm the buckets —
            # zero_grad(set_to_none=True) would detach every p.grad from the arena and no collective would ever run
            self.reducer.zero_grad()
            self.reducer.prepare(None)
        else:
            # gradients are zero-filled in place (one multi-tensor launch) rather than dropped: the native tower nodes ADD
            # their weight gradients into existing .grad tensors, and re-creating ~400 of them per step costs ~400 fills
            self.optimizer.zero_grad(set_to_none=False)
        if self.l0_optimizer is not None:
            self.l0_optimizer.zero_grad(set_to_none=True)
        loss = self.loss(images, texts)
        loss.backward()
        if self.reducer is not None:
            assert self.reducer.owns_grads(), "a parameter gradient no longer aliases the reducer's arena"
            self.reducer.finish()
        if self.clip is not None:
            self.last_grad_norm = grad_clip.clip_grad_norm_(self.params, self.clip)    # train.py:500 logs it (a device tensor)
        self.optimizer.step()
        if self.l0_optimizer is not None:
            self.l0_optimizer.step()
        for m in l0_modules(self.student):                                                 # train.py:509-520
            if m is not None:
                m.constrain_parameters()
        self.step_index += 1
        with torch.no_grad():                                                              # train.py:526-530
            if self.logit_scale is not None:
                self.student.logit_scale.fill_(math.log(self.logit_scale))
            else:
                self.student.logit_scale.clamp_(0, math.log(100))
        return loss.detach()
