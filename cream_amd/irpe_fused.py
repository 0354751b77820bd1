"""Fused iRPE attention (contextual rpe on q / k / v) — host side of csrc/irpe_attn.hip.

`attention(qkv, scale, rpe_q, rpe_k, rpe_v)` computes what `RPEAttention.forward` does between the
qkv and proj linears (iRPE/DeiT-with-iRPE/rpe_vision_transformer.py:68-97) in one launch forward and
two launches (+ one tiny table-gradient product per rpe) backward; nothing of size L^2 is written to
HBM.  It takes the (B, L, 3, H, 64) bf16 output of the qkv linear as it is (q, k, v are strided views)
and returns (B, L, H*64) ready for the proj linear.

`usable(...)` says whether a given RPEAttention configuration is covered: bf16 operands (autocast),
head_dim 64 or 32, each rpe either absent or an iRPE with at most 64 buckets (product: 50, euclidean /
quant: <= 64; cross: rows + cols as ONE table over the occurring bucket pairs, 50 in the zoo — iRPE_Cross.merged_table) —
contextual, or bias mode on q / k (the lookups are then the bias table itself, irpe.py:622-624) — or, with rpe on k ALONE,
at most 128 buckets (ratio 2.0 product: 81, DETR-with-iRPE's published recipe); with or without a key padding mask.
Everything else (fp32, head_dim 48, q / v tables above 64 buckets, more than 128 buckets) takes the composed path of
cream_amd.rpe_attention / cream_amd.detr_attention on the HIP rpe_index operator.

Two kernel families sit underneath (include/cream_amd.h): csrc/irpe_attn.hip (head_dim 64, <= 64 buckets, no mask — the
packed `attention` / `fwd_core` / `bwd_core` entry goes there whenever it can, unchanged) and csrc/irpe_attn_x.hip
(head_dim 32 | 64, row width 64 | 128, key padding mask, separate q / k / v of common strides: `attention_qkv` /
`fwd_core_x` / `bwd_core_x`).
"""
import ctypes
import os

import torch

from . import _lib, timing

_BYTES = {}          # (data_ptr, shape, device) -> (ids tensor kept alive, as-is uint8, transposed uint8)


def padded_len(L):
    return (L + 31) // 32 * 32


def bucket_bytes(ids):
    """int32 (L, L) bucket ids -> (NP x NP uint8 as is, NP x NP uint8 transposed), cached per table."""
    key = (ids.data_ptr(), tuple(ids.shape), str(ids.device))
    hit = _BYTES.get(key)
    if hit is not None:
        return hit[1], hit[2]
    assert ids.dtype == torch.int32 and ids.dim() == 2 and ids.is_contiguous() and ids.is_cuda
    Lq, Lk = ids.shape
    NP = padded_len(max(Lq, Lk))
    lib = _lib.load()
    outs = []
    with torch.cuda.device(ids.device):
        stream = torch.cuda.current_stream().cuda_stream
        for tr in (0, 1):
            dst = torch.empty((NP, NP), dtype=torch.uint8, device=ids.device)
            _lib.check(lib.cream_irpe_bucket_bytes(dst.data_ptr(), ids.data_ptr(), Lq, Lk, NP, tr, stream),
                       "cream_irpe_bucket_bytes")
            outs.append(dst)
    _BYTES[key] = (ids, outs[0], outs[1])
    return outs[0], outs[1]


def _term(rpe, L, device, hw=None):
    """-> (table parameter, head stride, query-major ids, key-major ids, nb, bias mode) of one rpe module; hw = (height,
    width) of a rectangular map (default: the square map of L tokens, with L - h * w skipped tokens)."""
    if rpe is None:
        return None
    from .irpe import iRPE_Cross
    h_, w_ = hw if hw is not None else (None, None)
    if type(rpe) is iRPE_Cross:          # rows + cols = one lookup over the occurring bucket pairs (irpe.py:758-760)
        ids, _, _, nb = rpe.merged_ids_for(L, device, h_, w_)
        asis, tr = bucket_bytes(ids)
        w = rpe.merged_table(L, device, h_, w_)  # differentiable: the table gradient reaches both parameters through it
        return w, (0 if w.shape[0] == 1 else w[0].numel()), asis, tr, nb, rpe.mode == "bias"
    ids = rpe.bucket_ids_for(L, device, h_, w_)
    asis, tr = bucket_bytes(ids)
    bias = rpe.mode == "bias"
    w = rpe.lookup_table_bias if bias else rpe.lookup_table_weight
    hs = 0 if w.shape[0] == 1 else w[0].numel()
    return w, hs, asis, tr, rpe.num_buckets, bias


MAX_NB_ANY = 64       # every subset of rpe on q / k / v
MAX_NB_K = 128        # rpe on k alone (csrc/irpe_attn_x.hip: the fp32 scatter rows of a second table do not fit at 128 columns)


def usable(qkv_dtype, device, head_dim, L, rpes, attn_drop_active=False, dropout_p=0.0, key_padding=False, hw=None):
    """True exactly for what the kernels implement: a device, bf16, head_dim 32 | 64, L <= 2048, every rpe an iRPE (or the
    cross method's merged table) in contextual / bias mode with fp32 contiguous tables and ONE bucket count for all
    terms: at most 64, or at most 128 when k is the only term.  `key_padding`: a (B, L) key padding mask will be passed
    (always implemented; the argument is part of the decision's signature); `hw`: rectangular map.
    (attention dropout does not exclude the fused path: the kernels regenerate the keep mask from a seed;
    `nn.Dropout(p=1.0)` is legal and stays on the composed path — the C ABI rejects dropout_p >= 1)"""
    if os.environ.get("CREAM_IRPE_FUSED", "1") == "0":
        return False
    if dropout_p >= 1.0:
        return False
    if device.type != "cuda" or qkv_dtype != torch.bfloat16 or head_dim not in (32, 64) or L > 2048:
        return False
    from .irpe import iRPE, iRPE_Cross
    h_, w_ = hw if hw is not None else (None, None)
    rpes = tuple(rpes)
    nbs = set()
    for r in rpes:
        if r is None:
            continue
        if type(r) is iRPE_Cross:
            parts, nb = (r.rp_rows, r.rp_cols), r.merged_ids_for(L, device, h_, w_)[3]
        else:
            parts, nb = (r,), r.num_buckets
        for m in parts:
            if type(m) is not iRPE or m.mode not in ("contextual", "bias"):
                return False
            w = m.lookup_table_bias if m.mode == "bias" else m.lookup_table_weight
            if w.dtype != torch.float32 or not w.is_contiguous():
                return False
        if nb > MAX_NB_K:
            return False
        nbs.add(nb)
    if len(nbs) > 1:
        return False
    if nbs and max(nbs) > MAX_NB_ANY:            # above 64 buckets: rpe on k alone
        return len(rpes) == 3 and rpes[0] is None and rpes[1] is not None and rpes[2] is None
    return True


def _desc(qkv, scale, terms, out, lse, sv):
    B, L, _, H, D = qkv.shape
    d = _lib.IrpeAttnDesc()
    _lib.set_packed_qkv(d, qkv)
    d.out, d.lse, d.sv = out.data_ptr(), lse.data_ptr(), (sv.data_ptr() if sv is not None else None)
    tq, tk, tv = terms
    nb = 1
    if tq is not None:                       # rpe_q: bucket_q[j][i] is key-major as stored
        d.idq, d.idq_t, nb = tq[3].data_ptr(), tq[2].data_ptr(), tq[4]
        if tq[5]:
            d.bq, d.bq_hs = tq[0].data_ptr(), tq[1]
        else:
            d.wq, d.wq_hs = tq[0].data_ptr(), tq[1]
    if tk is not None:
        d.idk, d.idk_t, nb = tk[2].data_ptr(), tk[3].data_ptr(), tk[4]
        if tk[5]:
            d.bk, d.bk_hs = tk[0].data_ptr(), tk[1]
        else:
            d.wk, d.wk_hs = tk[0].data_ptr(), tk[1]
    if tv is not None:
        d.wv, d.wv_hs, d.idv, d.idv_t, nb = tv[0].data_ptr(), tv[1], tv[2].data_ptr(), tv[3].data_ptr(), tv[4]
    d.B, d.H, d.L, d.NP, d.nb = B, H, L, padded_len(L), nb
    d.scale = scale
    return d


def dropout_keep_mask(seed, B, H, L):
    """The keep mask of the kernels' attention dropout as a (B, H, L, L) uint32 array of hash values: element (b, h, i, j)
    is kept iff value >= round(p * 2^32).  numpy restatement of `drop_key` / `drop_keep` in csrc/irpe_attn.hip (a 32-bit
    multiply-xorshift mix of a per-(b, h) key and (i << 16 | j)); used by the tests to build the reference."""
    import numpy as np

    def mix32(x):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(16)
        return x

    bh = np.arange(B * H, dtype=np.uint64)
    key = mix32(np.uint64(seed & 0xFFFFFFFF) ^ (((bh + np.uint64(1)) * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)))
    i = np.arange(L, dtype=np.uint64)[:, None]
    j = np.arange(L, dtype=np.uint64)[None, :]
    pair = (i << np.uint64(16)) | j
    return mix32(key[:, None, None] ^ pair[None]).astype(np.uint32).reshape(B, H, L, L)


def dropout_threshold(p):
    """round(p * 2^32) clamped to [1, 2^32 - 1] as the C ABI computes it (cream_irpe_attn_desc.dropout_p is a float)."""
    import numpy as np
    thr = float(np.float32(p)) * 4294967296.0
    return int(min(max(thr, 1.0), 4294967295.0))


_seed_gen = None


def _new_seed(device=None):
    """Seed of one in-kernel keep mask.  On a GPU it is derived from the device generator's (seed, offset) — the state
    torch.nn.Dropout itself consumes (rpe_vision_transformer.py:64, :91) — and advances that offset: masks follow
    torch.manual_seed, a second torch.manual_seed(s) with the SAME s replays them, and no number of the host stream is used
    (Mixup / the configuration sampler draw from it between layers).  Without a device generator: a dedicated host generator
    seeded from torch.initial_seed()."""
    global _seed_gen
    gens = getattr(torch.cuda, "default_generators", ())
    if torch.cuda.is_available() and len(gens):
        g = gens[torch.cuda.current_device() if device is None else torch.device(device).index or 0]
        if hasattr(g, "get_offset"):
            seed, off = int(g.initial_seed()), int(g.get_offset())
            g.set_offset(off + 4)                              # (multiples of 4: one Philox counter step, as a dropout launch takes)
            x = (seed * 0x9E3779B97F4A7C15 + (off + 1) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
            x ^= x >> 31
            return int(x % (2 ** 31 - 1))
    if _seed_gen is None or _seed_gen[0] != torch.initial_seed():
        g = torch.Generator()
        g.manual_seed(torch.initial_seed() ^ 0x5DEECE66D)
        _seed_gen = (torch.initial_seed(), g)
    return int(torch.randint(0, 2 ** 31 - 1, (1,), generator=_seed_gen[1]).item())


def _flops(B, H, L, n_terms, bwd, D=64, W=64):
    return (2.5 if bwd else 1.0) * 4.0 * B * H * L * L * D + (3 if bwd else 1) * n_terms * 2.0 * B * H * L * D * W


def fwd_core(qkv, scale, terms, drop_p=0.0, seed=0, causal=False):
    """One forward launch: qkv (B, L, 3, H, 64) bf16 -> (out (B, L, H*64), lse (B, H, L) fp32, sv (B, H, NP, 64) or None).
    `terms` = (_term(rpe_q), _term(rpe_k), _term(rpe_v)), each None when absent.  Outside autograd."""
    B, L, _, H, D = qkv.shape
    NP = padded_len(L)
    out = torch.empty((B, L, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=qkv.device)
    sv = torch.empty((B, H, NP, 64), dtype=qkv.dtype, device=qkv.device) if terms[2] is not None else None
    d = _desc(qkv, scale, terms, out, lse, sv)
    d.dropout_p, d.dropout_seed = float(drop_p), int(seed)
    d.causal = 1 if causal else 0
    n_terms = sum(t is not None for t in terms)
    with torch.cuda.device(qkv.device), timing.region("irpe_attn_fwd", flops=_flops(B, H, L, n_terms, False)):
        rc = _lib.load().cream_irpe_attn_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_irpe_attn_fwd")
    return out, lse, sv


def bwd_core(dout, qkv, out, lse, sv, scale, terms, drop_p=0.0, seed=0, causal=False, *, return_rows=False):
    """The backward launches of fwd_core: -> (dqkv (B, L, 3, H, 64), [d table of rpe_q, rpe_k, rpe_v] — each None or a tensor of the
    table's shape and dtype).  Outside autograd.  `return_rows`: also a dict of what the launches hand to each other — `delta`
    (B, H, NP) fp32 and the bf16 side rows `lkg`, `gg`, `dlk`, `dlq` (B, H, NP, 64), None where the term is absent (for the
    kernel tests)."""
    tq, tk, tv = terms
    if tv is None:
        sv = None
    B, L, _, H, D = qkv.shape
    NP = padded_len(L)
    dev = qkv.device
    dout = dout.contiguous()
    dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
    d = _desc(qkv, scale, terms, out, lse, sv)
    d.dropout_p, d.dropout_seed = float(drop_p), int(seed)
    d.causal = 1 if causal else 0
    d.dout = dout.data_ptr()
    _lib.set_packed_dqkv(d, dqkv)
    delta = torch.empty((B, H, NP), dtype=torch.float32, device=dev)
    rows = lambda: torch.empty((B, H, NP, 64), dtype=qkv.dtype, device=dev)      # noqa: E731
    lkg = dlk = gg = dlq = None
    d.delta = delta.data_ptr()
    if tk is not None:
        lkg, dlk = rows(), rows()
        d.lkg, d.dlk = lkg.data_ptr(), dlk.data_ptr()
    if tv is not None:
        gg = rows()
        d.gg = gg.data_ptr()
    if tq is not None:
        dlq = rows()
        d.dlq = dlq.data_ptr()
    lib = _lib.load()
    n_terms = sum(t is not None for t in terms)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        with timing.region("irpe_attn_bwd", flops=_flops(B, H, L, n_terms, True)):
            rc = lib.cream_irpe_attn_bwd(ctypes.byref(d), stream)
        _lib.check(rc, "cream_irpe_attn_bwd")

        def table_grad(x, xs, y, ys, mul):
            part = torch.empty((B, H, 64, 64), dtype=torch.float32, device=dev)
            _lib.check(lib.cream_irpe_table_grad(part.data_ptr(), x, xs[0], xs[1], xs[2], y, ys[0], ys[1], ys[2],
                                                 B, H, L, mul, stream), "cream_irpe_table_grad")
            return part.sum(0)                                   # (H, 64, 64)

        qs = qkv.stride()
        q_str, row_str = (qs[0], qs[1], qs[3]), (H * NP * 64, 64, NP * 64)
        do_str = (L * H * 64, H * 64, 64)
        es_q = qkv.element_size()
        grads = [None, None, None]
        if tq is not None and tq[5]:   # bias mode: d lookup_table_bias (H', nb) = the bucket gradient rows summed
            grads[0] = dlq[:, :, :L].sum((0, 2), dtype=torch.float32)
        elif tq is not None:    # d lookup_table_weight(rpe_q) (H', 64, nb) = (scale k)^T dlq
            grads[0] = table_grad(qkv.data_ptr() + qs[2] * es_q, q_str, dlq.data_ptr(), row_str, scale)
        if tk is not None and tk[5]:
            grads[1] = dlk[:, :, :L].sum((0, 2), dtype=torch.float32)
        elif tk is not None:    # (scale q)^T dlk
            grads[1] = table_grad(qkv.data_ptr(), q_str, dlk.data_ptr(), row_str, scale)
        if tv is not None:      # (H', nb, 64) = sv^T dout
            grads[2] = table_grad(sv.data_ptr(), row_str, dout.data_ptr(), do_str, 1.0)
    res = []
    for gpart, t, transposed in zip(grads, terms, (True, True, False)):
        if gpart is None:
            res.append(None)
            continue
        w, nb = t[0], t[4]
        if w.shape[0] == 1:
            gpart = gpart.sum(0, keepdim=True)
        if t[5]:
            res.append(gpart[:, :nb].to(w.dtype).contiguous())
            continue
        res.append((gpart[:, :, :nb] if transposed else gpart[:, :nb, :]).to(w.dtype).contiguous())
    if return_rows:
        return dqkv, res, dict(delta=delta, lkg=lkg, gg=gg, dlk=dlk, dlq=dlq)
    return dqkv, res


class _Fused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, scale, wq, wk, wv, terms, drop_p=0.0, seed=0):
        out, lse, sv = fwd_core(qkv, scale, terms, drop_p, seed)
        ctx.drop = (float(drop_p), int(seed))
        ctx.save_for_backward(qkv, out, lse, sv if sv is not None else lse)
        ctx.scale, ctx.terms = scale, terms
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, sv = ctx.saved_tensors
        dqkv, res = bwd_core(dout, qkv, out, lse, sv, ctx.scale, ctx.terms, *ctx.drop)
        return dqkv, None, res[0], res[1], res[2], None, None, None


_NO_TERMS = (None, None, None)


def plain_fwd(qkv, scale, causal=False):
    """Attention without any relative position term, forward only, outside autograd: qkv (B, L, 3, H, 64) bf16 ->
    (out (B, L, H*64) bf16, lse (B, H, L) fp32).  For callers that sequence their own backward (cream_amd.tinyclip.native)."""
    return fwd_core(qkv, scale, _NO_TERMS, causal=causal)[:2]


def plain_bwd(dout, qkv, out, lse, scale, causal=False):
    """Backward of plain_fwd: -> dqkv (B, L, 3, H, 64) bf16 (two launches)."""
    return bwd_core(dout, qkv, out, lse, None, scale, _NO_TERMS, causal=causal)[0]


def attention(qkv, scale, rpe_q, rpe_k, rpe_v, dropout_p=0.0, seed=None):
    """qkv (B, L, 3, H, D) bf16, D = 64 | 32 -> (B, L, H*D).  dropout_p > 0: attention dropout inside the kernels
    (rpe_vision_transformer.py:86); `seed` (default: drawn from torch's host generator) fixes the keep mask, which
    `dropout_keep_mask` reproduces.  head_dim 64 with at most 64 buckets runs the kernels of csrc/irpe_attn.hip as before;
    head_dim 32 or more than 64 buckets goes through `attention_qkv`."""
    assert qkv.dim() == 5 and qkv.shape[2] == 3 and qkv.shape[4] in (32, 64) and qkv.stride(4) == 1
    L, dev = qkv.shape[1], qkv.device
    terms = tuple(_term(r, L, dev) for r in (rpe_q, rpe_k, rpe_v))
    if qkv.shape[4] != 64 or row_width(terms) != 64:
        return attention_qkv(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale, rpe_q, rpe_k, rpe_v, dropout_p=dropout_p, seed=seed)
    ws = [t[0] if t is not None else None for t in terms]
    if dropout_p and seed is None:
        seed = _new_seed(dev)
    return _Fused.apply(qkv, float(scale), ws[0], ws[1], ws[2], terms, float(dropout_p or 0.0), int(seed or 0))


# ---- head_dim 32 | 64, up to 128 buckets on k, key padding mask, separate q / k / v (csrc/irpe_attn_x.hip) ------------

def row_width(terms):
    """Width of the bucket-indexed side rows (sv, lkg, gg, dlk, dlq) for these terms: 64, or 128 above 64 buckets."""
    nb = max([t[4] for t in terms if t is not None], default=1)
    return 64 if nb <= 64 else 128


def _pad_bytes(key_padding_mask, B, L):
    if key_padding_mask is None:
        return None
    assert key_padding_mask.shape == (B, L), (tuple(key_padding_mask.shape), (B, L))
    m = key_padding_mask
    return (m if m.dtype == torch.uint8 else m.ne(0).to(torch.uint8)).contiguous()


def _desc_x(q, k, v, scale, terms, out, lse, sv, pad, seq_first):
    """q, k, v: (B, L, H, D) bf16 views with COMMON strides and unit stride over D; out (B, L, H*D) or, seq_first,
    (L, B, H*D) contiguous."""
    B, L, H, D = q.shape
    assert k.shape == q.shape and v.shape == q.shape and q.stride() == k.stride() == v.stride() and q.stride(3) == 1
    x = _lib.IrpeAttn2Desc()
    d = x.base
    d.q, d.k, d.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    d.sb, d.sn, d.sh = q.stride(0), q.stride(1), q.stride(2)
    d.out, d.lse, d.sv = out.data_ptr(), lse.data_ptr(), (sv.data_ptr() if sv is not None else None)
    tq, tk, tv = terms
    nb = 1
    if tq is not None:                       # rpe_q: bucket_q[j][i] is key-major as stored
        d.idq, d.idq_t, nb = tq[3].data_ptr(), tq[2].data_ptr(), tq[4]
        if tq[5]:
            d.bq, d.bq_hs = tq[0].data_ptr(), tq[1]
        else:
            d.wq, d.wq_hs = tq[0].data_ptr(), tq[1]
    if tk is not None:
        d.idk, d.idk_t, nb = tk[2].data_ptr(), tk[3].data_ptr(), tk[4]
        if tk[5]:
            d.bk, d.bk_hs = tk[0].data_ptr(), tk[1]
        else:
            d.wk, d.wk_hs = tk[0].data_ptr(), tk[1]
    if tv is not None:
        d.wv, d.wv_hs, d.idv, d.idv_t, nb = tv[0].data_ptr(), tv[1], tv[2].data_ptr(), tv[3].data_ptr(), tv[4]
    d.B, d.H, d.L, d.NP, d.nb = B, H, L, padded_len(L), nb
    d.scale = scale
    x.head_dim, x.row_width = D, row_width(terms)
    if pad is not None:
        x.key_pad, x.key_pad_sb = pad.data_ptr(), L
    x.osb, x.osn = (H * D, B * H * D) if seq_first else (L * H * D, H * D)
    x.dosb, x.dosn = x.osb, x.osn
    return x


def fwd_core_x(q, k, v, scale, terms, key_pad=None, drop_p=0.0, seed=0, causal=False, seq_first=False):
    """One forward launch: q, k, v (B, L, H, D) bf16 views of common strides, D = 32 | 64; key_pad (B, L) uint8 or None
    -> (out (B, L, H*D) — or (L, B, H*D) when seq_first —, lse (B, H, L) fp32, sv (B, H, NP, row width) or None).
    Outside autograd."""
    B, L, H, D = q.shape
    NP, W = padded_len(L), row_width(terms)
    out = torch.empty((L, B, H * D) if seq_first else (B, L, H * D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device)
    sv = torch.empty((B, H, NP, W), dtype=q.dtype, device=q.device) if terms[2] is not None else None
    x = _desc_x(q, k, v, scale, terms, out, lse, sv, key_pad, seq_first)
    x.base.dropout_p, x.base.dropout_seed = float(drop_p), int(seed)
    x.base.causal = 1 if causal else 0
    n_terms = sum(t is not None for t in terms)
    with torch.cuda.device(q.device), timing.region("irpe_attn_fwd", flops=_flops(B, H, L, n_terms, False, D, W)):
        rc = _lib.load().cream_irpe_attn2_fwd(ctypes.byref(x), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cream_irpe_attn2_fwd")
    return out, lse, sv


def bwd_core_x(dout, q, k, v, out, lse, sv, scale, terms, key_pad=None, drop_p=0.0, seed=0, causal=False, seq_first=False,
               partials=None, *, return_rows=False):
    """The backward launches of fwd_core_x: -> ((dq, dk, dv) as (B, L, H, D) views of one buffer laid out like `out`,
    [d table of rpe_q, rpe_k, rpe_v]).  `partials`: a dict that receives the per-image table-gradient partials
    (B, H, ., .) before their reduction over the batch (tests).  Outside autograd.  `return_rows`: also a dict of `delta`
    (B, H, NP) fp32 and the bf16 side rows `lkg`, `gg`, `dlk`, `dlq` (B, H, NP, row width), None where the term is absent
    (for the kernel tests)."""
    tq, tk, tv = terms
    if tv is None:
        sv = None
    B, L, H, D = q.shape
    NP, W = padded_len(L), row_width(terms)
    dev = q.device
    dout = dout.contiguous()
    x = _desc_x(q, k, v, scale, terms, out, lse, sv, key_pad, seq_first)
    d = x.base
    d.dropout_p, d.dropout_seed = float(drop_p), int(seed)
    d.causal = 1 if causal else 0
    d.dout = dout.data_ptr()
    if seq_first:
        d3 = torch.empty((3, L, B, H, D), dtype=q.dtype, device=dev)
        dq, dk, dv = (d3[i].permute(1, 0, 2, 3) for i in range(3))
    else:
        d3 = torch.empty((3, B, L, H, D), dtype=q.dtype, device=dev)
        dq, dk, dv = d3[0], d3[1], d3[2]
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.dsb, d.dsn, d.dsh = dq.stride(0), dq.stride(1), dq.stride(2)
    delta = torch.empty((B, H, NP), dtype=torch.float32, device=dev)
    rows = lambda: torch.empty((B, H, NP, W), dtype=q.dtype, device=dev)      # noqa: E731
    lkg = dlk = gg = dlq = None
    d.delta = delta.data_ptr()
    if tk is not None:
        lkg, dlk = rows(), rows()
        d.lkg, d.dlk = lkg.data_ptr(), dlk.data_ptr()
    if tv is not None:
        gg = rows()
        d.gg = gg.data_ptr()
    if tq is not None:
        dlq = rows()
        d.dlq = dlq.data_ptr()
    lib = _lib.load()
    n_terms = sum(t is not None for t in terms)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        with timing.region("irpe_attn_bwd", flops=_flops(B, H, L, n_terms, True, D, W)):
            rc = lib.cream_irpe_attn2_bwd(ctypes.byref(x), stream)
        _lib.check(rc, "cream_irpe_attn2_bwd")

        def table_grad(name, xt, xs, xa, yt, ys, yc, mul):
            part = torch.empty((B, H, xa, yc), dtype=torch.float32, device=dev)
            _lib.check(lib.cream_irpe_table_grad2(part.data_ptr(), xt.data_ptr(), xs[0], xs[1], xs[2], xa, yt.data_ptr(),
                                                  ys[0], ys[1], ys[2], yc, B, H, L, mul, stream), "cream_irpe_table_grad2")
            if partials is not None:
                partials[name] = part
            return part.sum(0)                                   # (H, xa, yc)

        def bias_grad(name, r):
            part = r[:, :, :L].sum(2, dtype=torch.float32)       # (B, H, W)
            if partials is not None:
                partials[name] = part
            return part.sum(0)

        q_str, row_str = q.stride()[:3], (H * NP * W, W, NP * W)
        do_str = (x.dosb, x.dosn, D)
        grads = [None, None, None]
        if tq is not None and tq[5]:   # bias mode: d lookup_table_bias (H', nb) = the bucket gradient rows summed
            grads[0] = bias_grad("q", dlq)
        elif tq is not None:    # d lookup_table_weight(rpe_q) (H', D, nb) = (scale k)^T dlq
            grads[0] = table_grad("q", k, q_str, D, dlq, row_str, W, scale)
        if tk is not None and tk[5]:
            grads[1] = bias_grad("k", dlk)
        elif tk is not None:    # (scale q)^T dlk
            grads[1] = table_grad("k", q, q_str, D, dlk, row_str, W, scale)
        if tv is not None:      # (H', nb, D) = sv^T dout
            grads[2] = table_grad("v", sv, row_str, W, dout, do_str, D, 1.0)
    res = []
    for gpart, t, transposed in zip(grads, terms, (True, True, False)):
        if gpart is None:
            res.append(None)
            continue
        w, nb = t[0], t[4]
        if w.shape[0] == 1:
            gpart = gpart.sum(0, keepdim=True)
        if t[5]:
            res.append(gpart[:, :nb].to(w.dtype).contiguous())
            continue
        res.append((gpart[:, :, :nb] if transposed else gpart[:, :nb, :]).to(w.dtype).contiguous())
    if return_rows:
        return (dq, dk, dv), res, dict(delta=delta, lkg=lkg, gg=gg, dlk=dlk, dlq=dlq)
    return (dq, dk, dv), res


class _FusedX(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, wq, wk, wv, terms, key_pad, drop_p, seed, seq_first):
        out, lse, sv = fwd_core_x(q, k, v, scale, terms, key_pad, drop_p, seed, seq_first=seq_first)
        ctx.save_for_backward(q, k, v, out, lse, sv if sv is not None else lse)
        ctx.args = (scale, terms, key_pad, float(drop_p), int(seed), seq_first)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, sv = ctx.saved_tensors
        scale, terms, key_pad, drop_p, seed, seq_first = ctx.args
        (dq, dk, dv), res = bwd_core_x(dout, q, k, v, out, lse, sv, scale, terms, key_pad, drop_p, seed, seq_first=seq_first)
        return dq, dk, dv, None, res[0], res[1], res[2], None, None, None, None, None


def attention_qkv(q, k, v, scale, rpe_q, rpe_k, rpe_v, key_padding_mask=None, dropout_p=0.0, seed=None, hw=None,
                  seq_first=False):
    """Fused iRPE attention on separate q, k, v: (B, L, H, D) bf16 views with COMMON strides (e.g. slices of one packed
    projection, or three projections of the same layout), D = 32 | 64 -> (B, L, H*D); with seq_first the result is
    allocated and returned sequence-first, (L, B, H*D), for callers whose tensors are (L, N, E).  The logits are
    (scale q) . k + rpe_k(scale q) + rpe_q(scale k)^T as in `attention`.  key_padding_mask (B, L) bool / byte: non-zero
    = that key takes no part for any query of its image (at least one real key per image).  hw: (height, width) of a
    rectangular map.  The caller checks `usable(...)` first; what the kernels do not implement raises."""
    assert q.dim() == 4 and q.shape[3] in (32, 64) and q.stride(3) == 1
    B, L, dev = q.shape[0], q.shape[1], q.device
    terms = tuple(_term(r, L, dev, hw) for r in (rpe_q, rpe_k, rpe_v))
    ws = [t[0] if t is not None else None for t in terms]
    if dropout_p and seed is None:
        seed = _new_seed(dev)
    pad = _pad_bytes(key_padding_mask, B, L)
    return _FusedX.apply(q, k, v, float(scale), ws[0], ws[1], ws[2], terms, pad, float(dropout_p or 0.0), int(seed or 0),
                         bool(seq_first))
