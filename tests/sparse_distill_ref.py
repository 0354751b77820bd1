"""Plain float64 restatements of the two contracts of csrc/sparse_distill.hip (include/cream_amd.h: cream_sparse_ce,
cream_softmax_topk_records) and the input builder of their tests.  Nothing here shares code with the kernels or with
cream_amd/tinyvit_distill.py.  tests/test_sparse_distill_ref_cpu.py pins these against the framework's float64 operators,
tests/test_sparse_distill_kernel_gpu.py holds the kernels to them."""
import numpy as np
import torch


# ---- cream_sparse_ce --------------------------------------------------------------------------------------------------
def dense_target(index, value, C):
    """t (B, C) float64: value[b, j] at class index[b, j], (1 - sum_j value[b, j]) / (C - k) at every other class."""
    B, k = index.shape
    v = value.double()
    t = ((1.0 - v.sum(-1, keepdim=True)) / (C - k)).expand(B, C).clone()
    rows = torch.arange(B, device=index.device)[:, None].expand(B, k)
    t[rows, index.long()] = v
    return t


def sparse_ce(logits, index, value, grad_scale):
    """loss_rows (B) = sum_c t (lse - x_c) and dlogits (B, C) = (softmax(x) sum_c t - t) * grad_scale in float64."""
    x = logits.double()
    t = dense_target(index, value, x.shape[1])
    mx = x.max(-1, keepdim=True).values
    e = torch.exp(x - mx)
    se = e.sum(-1, keepdim=True)
    lse = mx + se.log()
    return (t * (lse - x)).sum(-1), (e / se * t.sum(-1, keepdim=True) - t) * grad_scale


def sparse_ce_closed_form(logits, index, value):
    """The form the kernel's header states, in float64: minor * sum over the unpatched classes of (lse - x_c) plus
    sum_j v_j (lse - x_{index_j})."""
    x, v, idx = logits.double(), value.double(), index.long()
    B, C = x.shape
    k = idx.shape[1]
    lse = torch.logsumexp(x, -1, keepdim=True)
    minor = (1.0 - v.sum(-1)) / (C - k)
    terms = lse - x
    patched = torch.gather(terms, 1, idx)
    return minor * (terms.sum(-1) - patched.sum(-1)) + (v * patched).sum(-1)


# ---- cream_softmax_topk_records -------------------------------------------------------------------------------------------
def topk_order(logits, k):
    """The order rule: larger logit first, equal logits by ascending class index.  (B, k) int64 numpy."""
    x = logits.detach().double().cpu().numpy()
    return np.stack([np.argsort(-row, kind="stable")[:k] for row in x])


def softmax64(logits):
    return torch.softmax(logits.double(), -1)


def fp16_value_ok(h, r, eps):
    """h (fp16 array) is the round-to-nearest of SOME real within relative eps of r (float64 array): the interval of reals
    that round to h — half way to either fp16 neighbour — meets [r (1 - eps), r (1 + eps)].  Elementwise bool."""
    h16 = np.asarray(h, dtype=np.float16)
    hf = h16.astype(np.float64)
    below = np.nextafter(h16, np.float16(-np.inf)).astype(np.float64)
    above = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
    lo, hi = (hf + below) / 2, (hf + above) / 2
    r = np.asarray(r, dtype=np.float64)
    return (lo <= r * (1 + eps)) & (hi >= r * (1 - eps)) & np.isfinite(hf)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def build_topk_logits(B, C, k, seed, step=1.0 / 16):
    """(B, C) float32 logits, every value exact in bf16: the top k + 1 are the distinct values 6 - j * step (j = 0 .. k; step
    1/16 keeps neighbouring probabilities 6 % apart, step 1/8 with k = 100 pushes the tail below 2^-14), the rest are multiples
    of 1/4 clamped below them, with many ties among themselves; positions permuted per row."""
    g = torch.Generator().manual_seed(seed)
    top = 6.0 - torch.arange(min(k + 1, C), dtype=torch.float32) * step
    ceiling = float(torch.floor(top[-1] * 4) / 4) - 0.25
    x = torch.empty(B, C)
    for b in range(B):
        rest = torch.clamp(torch.round(torch.randn(C - len(top), generator=g) * 8) / 4, max=0.0) + ceiling
        row = torch.cat([top, rest])
        x[b] = row[torch.randperm(C, generator=g)]
    assert torch.equal(x.bfloat16().float(), x)
    return x


def build_records(B, C, k, seed, total=0.9):
    """Distinct random classes per row and fp16 values that sum to about `total` (above 1: `minor` < 0)."""
    g = torch.Generator().manual_seed(seed)
    index = torch.stack([torch.randperm(C, generator=g)[:k] for _ in range(B)]).to(torch.int16)
    value = (torch.softmax(torch.randn(B, k, generator=g) * 2, -1).sort(-1, descending=True).values * total).to(torch.float16)
    return index, value
