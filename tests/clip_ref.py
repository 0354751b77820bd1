"""Float64 restatement of global-norm gradient clipping (torch.nn.utils.clip_grad_norm_ with norm_type 2), written out from
its definition for the tests of cream_amd/grad_clip.py and of the clip kernels of csrc/optim.hip.  Shares no code with the
product; pinned against the framework function on float64 tensors in tests/test_grad_clip_cpu.py."""
import math

import torch


def clip(grads, max_norm):
    """(norm, coef, scaled gradients): norm = sqrt(sum of every squared element), coef = min(1, max_norm / (norm + 1e-6)),
    all in float64 (norm and coef as Python floats)."""
    g64 = [g.detach().double() for g in grads]
    total = 0.0
    for g in g64:
        total += float((g * g).sum())
    norm = math.sqrt(total)
    coef = min(1.0, max_norm / (norm + 1e-6))
    return norm, coef, [g * coef for g in g64]
