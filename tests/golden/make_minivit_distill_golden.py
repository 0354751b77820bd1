"""Golden vectors of the Mini-Swin distillation step, made by the reference's own classes and functions
(MiniViT/Mini-Swin/models/swin_transformer_minivit_distill.py `SwinTransformerMiniViTDistill`, swin_transformer_distill.py
`SwinTransformerDISTILL`, and `soft_cross_entropy`, `cal_relation_loss`, `cal_hidden_loss`, `cal_hidden_relation_loss` of
main.py), loaded read-only with the timm stand-ins of tests/refshim.py:
    python tests/golden/make_minivit_distill_golden.py        ->  tests/golden/minivit_distill.{npz,json}
The two model files import their siblings relatively, so they are loaded under a synthetic parent package whose __path__ is
the reference's models directory; main.py imports packages a test machine need not have, so the four loss functions are taken
out of its syntax tree.  Student: the two-stage Mini-Swin of make_miniswin_golden.py with the three flags on, is_student and
fit_size_C = 96; teacher: a plain two-stage Swin of width 96.  Both tap layers [1, 3]: the shifted four-window repeat of stage
one and the second single-window repeat of stage two.  Seeded weights (`miniswin_fill`) and inputs; per `is_hidden_org`
setting the files hold the logits, the loss values and per student parameter the gradient's norm, sum and a strided sample of
the total loss (soft + relation + hidden) — no weights."""
import ast
import contextlib
import importlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
from make_miniswin_golden import MODEL, STRIDE, digest, inputs, miniswin_fill  # noqa: E402,F401

STUDENT = dict(MODEL, is_sep_layernorm=True, is_transform_FFN=True, is_transform_heads=True, is_student=True, fit_size_C=96)
TEACHER = dict(img_size=56, patch_size=4, embed_dim=96, depths=[2, 2], num_heads=[3, 6], window_size=7, drop_path_rate=0.0)
LAYERS = [1, 3]
SEEDS = dict(student=29, teacher=31)
LOSS_FUNCTIONS = ("soft_cross_entropy", "cal_relation_loss", "cal_hidden_loss", "cal_hidden_relation_loss")
SETTINGS = {"hidden_org": True, "hidden_fit": False}            # tag -> is_hidden_org


def load_reference():
    """-> (make_student, make_teacher, {name: loss function})."""
    import refshim
    assert refshim.have_reference(), "needs the reference checkout"
    refshim._install_timm_stub()
    root = os.path.join(refshim.REFERENCE, "MiniViT", "Mini-Swin")
    pkg = types.ModuleType("_ref_miniswin_models")
    pkg.__path__ = [os.path.join(root, "models")]
    sys.modules[pkg.__name__] = pkg
    student_mod = importlib.import_module(pkg.__name__ + ".swin_transformer_minivit_distill")
    teacher_mod = importlib.import_module(pkg.__name__ + ".swin_transformer_distill")
    tree = ast.parse(open(os.path.join(root, "main.py")).read())
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in LOSS_FUNCTIONS]
    assert len(picked) == len(LOSS_FUNCTIONS)
    ns = {"torch": torch}
    exec(compile(ast.Module(body=picked, type_ignores=[]), "main.py", "exec"), ns)

    def quiet(cls):
        def make(**kw):
            with contextlib.redirect_stdout(io.StringIO()):          # the constructors print their drop-path lists
                return cls(**kw)
        return make
    return quiet(student_mod.SwinTransformerMiniViTDistill), quiet(teacher_mod.SwinTransformerDISTILL), {k: ns[k] for k in LOSS_FUNCTIONS}


def main():
    import warnings
    warnings.simplefilter("ignore")
    make_student, make_teacher, fn = load_reference()
    torch.manual_seed(0)
    student = make_student(**STUDENT)
    teacher = make_teacher(**TEACHER)
    miniswin_fill(student, seed=SEEDS["student"])
    miniswin_fill(teacher, seed=SEEDS["teacher"])
    student.eval()
    teacher.eval()
    x, _ = inputs("distill")
    outs, meta = {}, {}
    for name, m in (("student", student), ("teacher", teacher)):
        sd = m.state_dict()
        meta[name] = dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()],
                          n_params=sum(p.numel() for p in m.parameters()))
    with torch.no_grad():
        logits_t, qkv_t, hidden_t = teacher(x, LAYERS, is_attn_loss=True, is_hidden_loss=True)
    outs["teacher|logits"] = logits_t.numpy()
    meta["tap_shapes"] = dict(teacher_qkv=[list(t[0].shape) for t in qkv_t], teacher_hidden=[list(h.shape) for h in hidden_t])
    for tag, org in SETTINGS.items():
        student.zero_grad(set_to_none=True)
        logits, qkv_s, hidden_s = student(x, LAYERS, is_attn_loss=True, is_hidden_loss=True, is_hidden_org=org)
        soft = fn["soft_cross_entropy"](logits, logits_t)
        attn = fn["cal_relation_loss"](qkv_s, qkv_t, 1)
        hidden = (fn["cal_hidden_relation_loss"] if org else fn["cal_hidden_loss"])(hidden_s, hidden_t)
        total = soft + attn + hidden
        total.backward()
        grads = {k: p.grad for k, p in student.named_parameters() if p.grad is not None}
        meta["tap_shapes"][tag] = dict(qkv=[list(t[0].shape) for t in qkv_s], hidden=[list(h.shape) for h in hidden_s],
                                       no_grad=sorted(k for k, p in student.named_parameters() if p.grad is None))
        outs[f"{tag}|logits"] = logits.detach().numpy()
        for k, v in dict(soft=soft, attn=attn, hidden=hidden, total=total).items():
            outs[f"{tag}|loss|{k}"] = v.detach().double().reshape(1).numpy()
        for k, v in digest(grads).items():
            outs[f"{tag}|{k}"] = v.numpy()
    json.dump(meta, open(os.path.join(HERE, "minivit_distill.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "minivit_distill.npz"), **outs)
    print("wrote minivit_distill.npz", os.path.getsize(os.path.join(HERE, "minivit_distill.npz")), "bytes")


if __name__ == "__main__":
    main()
