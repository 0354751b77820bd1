"""Global-norm gradient clipping — `torch.nn.utils.clip_grad_norm_` with norm_type 2 — on the kernels of csrc/optim.hip.

The recipes this package mirrors clip right in front of the optimizer (TinyCLIP/src/training/train.py:500 at 5, DETR's
engine.py:55 at 0.1, `loss_scaler(..., clip_grad=max_norm)` of AutoFormer/supernet_engine.py:96).  The framework routine is a
multi-tensor norm, a stack + norm and a multi-tensor multiply over every gradient; here it is one deterministic reduction
over a device-resident job table (two launches) and one in-place scale that loads nothing when the coefficient is 1 — and
no host synchronisation: the returned norm is a device tensor.  (`NativeAdamW.step(max_norm=...)` goes one further and folds
the multiply into the update.)

Which path runs is decided from the inputs alone: contiguous fp32 CUDA gradients on one device take the kernels, anything
else (CPU, bf16 / fp16, non-contiguous, several devices, a parameter without gradient, an empty list, a gradient that does not
start on a 16-byte boundary — the kernels load four floats at a time) the framework function.
"""
import torch

from .autoformer import block as _block

_cache = {}                                  # device -> (gradient pointers, shapes), JobTable


def _device_grads(params):
    grads = []
    for p in params:
        g = p.grad
        if (g is None or not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() or g.numel() == 0
                or g.data_ptr() % 16 or (grads and g.device != grads[0].device)):
            return None
        grads.append(g)
    return grads or None


def table_for(grads):
    """The cached table of gradient-only jobs (p == NULL: the norm and scale kernels read g, rows, cols, ld alone), rebuilt
    when a gradient tensor was replaced."""
    key = tuple((g.data_ptr(), tuple(g.shape)) for g in grads)
    dev = grads[0].device
    hit = _cache.get(dev)
    if hit is None or hit[0] != key:
        jobs = []
        for g in grads:
            j = _block.param_job(g, grad=g)
            j.p = 0
            jobs.append(j)
        hit = _cache[dev] = (key, _block.JobTable(jobs, dev))
    return hit[1]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm):
    """Scales the gradients in place by min(1, max_norm / (norm + 1e-6)) and returns the norm before clipping (a device
    tensor on the kernel path: reading it is the caller's synchronisation)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    grads = _device_grads(params)
    if grads is None or not float(max_norm) > 0.0:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0)
    with torch.cuda.device(grads[0].device):
        table = table_for(grads)
        out = table.clip_coef(max_norm)
        table.scale_grads(out[1:])
    return out[0]
