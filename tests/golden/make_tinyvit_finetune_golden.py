"""Golden record of TinyViT's fine-tune optimizer set-up, made by the reference's own code (TinyViT/models/tiny_vit.py,
TinyViT/optimizer.py and TinyViT/tinyvit_utils.py, loaded read-only as stand-alone modules; optimizer.py finds
`tinyvit_utils` under that name):
    python tests/golden/make_tinyvit_finetune_golden.py        ->  tests/golden/tinyvit_finetune.json
The small MODEL of make_tinyvit_golden.py with layer_lr_decay 0.8 goes through the reference's `build_optimizer` (AdamW,
BASE_LR 2.5e-4, WEIGHT_DECAY 1e-8 — the 22k -> 1k recipes) and its `LRSchedulerWrapper` around `WarmupCosine`, the stand-in
below for timm's CosineLRScheduler (timm is not installed), which the tests reuse.  The file holds, per parameter group, the
`param_name`s in order, `weight_decay` (null where the group has no such key before the optimizer fills its default) and
`lr_scale`; every group's `lr` before any scheduler call and after step_update(0), step_update(1) and step_update(7)."""
import json
import math
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
from make_tinyvit_golden import MODEL, load_reference  # noqa: E402

LAYER_LR_DECAY = 0.8
BASE_LR, WEIGHT_DECAY, BETAS, EPS = 2.5e-4, 1e-8, (0.9, 0.999), 1e-8
UPDATES = (0, 1, 7)


class WarmupCosine:
    """A cosine schedule with linear warm-up that writes ONE value into every group's `lr` — what timm's CosineLRScheduler
    does per update (t_in_epochs False), warm-up rate written at construction included."""

    def __init__(self, optimizer, base_lr, t_initial=20, warmup_t=4, warmup_lr_init=None, lr_min=None):
        self.optimizer, self.base_lr, self.t_initial, self.warmup_t = optimizer, base_lr, t_initial, warmup_t
        self.warmup_lr_init = base_lr * 1e-3 if warmup_lr_init is None else warmup_lr_init
        self.lr_min = base_lr * 1e-2 if lr_min is None else lr_min
        self.last = None
        self._write(self.warmup_lr_init)

    def _write(self, lr):
        for group in self.optimizer.param_groups:
            group['lr'] = lr

    def lr_at(self, it):
        if it < self.warmup_t:
            return self.warmup_lr_init + it * (self.base_lr - self.warmup_lr_init) / self.warmup_t
        frac = (it - self.warmup_t) / (self.t_initial - self.warmup_t)
        return self.lr_min + 0.5 * (self.base_lr - self.lr_min) * (1.0 + math.cos(math.pi * frac))

    def step(self, epoch):                       # (per-update schedule: an epoch boundary changes nothing)
        pass

    def step_update(self, it):
        self.last = it
        self._write(self.lr_at(it))

    def state_dict(self):
        return {'last': self.last}

    def load_state_dict(self, sd):
        self.last = sd['last']


def load_reference_optimizer():
    """(optimizer.py, tinyvit_utils.py) of the reference as modules."""
    import importlib.util
    import refshim
    out = []
    for name, file in (("tinyvit_utils", "tinyvit_utils.py"), ("_ref_tinyvit_optimizer", "optimizer.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(refshim.REFERENCE, "TinyViT", file))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        out.append(mod)
    return out[1], out[0]


def lrs(optimizer):
    return [g['lr'] for g in optimizer.param_groups]


def main():
    import warnings
    warnings.simplefilter("ignore")
    ref = load_reference()
    ref_opt, ref_utils = load_reference_optimizer()
    torch.manual_seed(0)
    model = ref.TinyViT(**dict(MODEL, layer_lr_decay=LAYER_LR_DECAY))
    config = types.SimpleNamespace(TRAIN=types.SimpleNamespace(
        BASE_LR=BASE_LR, WEIGHT_DECAY=WEIGHT_DECAY, OPTIMIZER=types.SimpleNamespace(NAME='adamw', EPS=EPS, BETAS=BETAS)))
    # the groups as the optimizer receives them (weight_decay absent in the decayed ones): the reference's two helpers
    skip_keywords = model.no_weight_decay_keywords()
    raw = ref_utils.divide_param_groups_by_lr_scale(ref_opt.set_weight_decay(model, {}, skip_keywords))
    optimizer = ref_opt.build_optimizer(config, model)
    assert isinstance(optimizer, torch.optim.AdamW) and len(optimizer.param_groups) == len(raw)
    groups = []
    for g, r in zip(optimizer.param_groups, raw):
        assert [id(p) for p in g['params']] == [id(p) for p in r['params']]
        groups.append(dict(params=[p.param_name for p in g['params']], weight_decay=r.get('weight_decay'),
                           weight_decay_in_optimizer=g['weight_decay'], lr_scale=g['lr_scale']))
    record = dict(model=dict(MODEL, layer_lr_decay=LAYER_LR_DECAY), base_lr=BASE_LR, weight_decay=WEIGHT_DECAY, groups=groups,
                  lr_at_construction=lrs(optimizer))
    scheduler = ref_utils.LRSchedulerWrapper(WarmupCosine(optimizer, BASE_LR), optimizer)
    record['lr_before_any_call'] = lrs(optimizer)
    for it in UPDATES:
        scheduler.step_update(it)
        record[f'lr_after_step_update_{it}'] = lrs(optimizer)
    path = os.path.join(HERE, 'tinyvit_finetune.json')
    json.dump(record, open(path, 'w'), indent=None, separators=(',', ':'))
    print("wrote tinyvit_finetune.json", os.path.getsize(path), "bytes;", len(groups), "groups")


if __name__ == "__main__":
    main()
