"""What the pruned-tower tests share (tests/test_tinyclip_pruned_cpu.py, tests/test_pruned_kernel_gpu.py,
tests/test_tinyclip_pruned_gpu.py): a NumPy restatement of the gradient finalisation's summation tree (csrc/grad_tree.hpp) and
of pad / unpad, and the toy tower pruned by hand-set 0 / 1 masks."""
import numpy as np


# ---- the summation tree of cream_grad_finalize / cream_grad_finalize_compact ------------------------------------------------
def part_lanes(nparts):
    return 4 if nparts <= 16 else (16 if nparts <= 64 else 64)


def tree_sum(parts):
    """parts (nparts, ...) fp32 -> (...) fp32: part lane l adds parts l, l + PL, ... in ascending order (from zero); the lanes
    are added in ascending order — for PL = 64 in 8 groups of 8 lanes, then the 8 group sums.  Every addition in fp32."""
    parts = np.asarray(parts, dtype=np.float32)
    n = parts.shape[0]
    PL = part_lanes(n)
    lanes = []
    for l in range(PL):
        acc = np.zeros(parts.shape[1:], dtype=np.float32)
        for p in range(l, n, PL):
            acc = acc + parts[p]
        lanes.append(acc)
    if PL == 64:
        groups = []
        for g in range(8):
            s = lanes[8 * g]
            for l in range(1, 8):
                s = s + lanes[8 * g + l]
            groups.append(s)
        lanes = groups
    s = lanes[0]
    for l in range(1, len(lanes)):
        s = s + lanes[l]
    return s


def finalize_compact(dst, src, rows, cols, ld_src, overwrite):
    """dst (rows, cols) fp32, src (nparts, >= rows, ld_src) -> what cream_grad_finalize_compact leaves in dst."""
    s = tree_sum(np.asarray(src, dtype=np.float32)[:, :rows, :cols])
    return s if overwrite else np.asarray(dst, dtype=np.float32) + s


def pad_cols(x, Dp):
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros((x.shape[0], Dp), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def unpad_cols(x, d):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)[:, :d])


# ---- the toy tower ------------------------------------------------------------------------------------------------------------
WIDTH, LAYERS, HEADS = 128, 5, 2
HEADS_KEPT = [2, 1, 0, 2, 0]
INTER_KEPT = [509, 64, 8, 512, 100]
FFN_Z = [1.0, 1.0, 1.0, 0.0, 0.0]           # layer 2 loses attention (no head left), layer 3 the MLP, layer 4 both


def toy_masks(hidden_keep):
    import torch
    g = torch.Generator().manual_seed(17)
    zh = torch.zeros(WIDTH)
    zh[torch.randperm(WIDTH, generator=g)[:hidden_keep]] = 1.0
    zd = torch.zeros(LAYERS, HEADS)
    zi = torch.zeros(LAYERS, 4 * WIDTH)
    for i in range(LAYERS):
        zd[i, HEADS - HEADS_KEPT[i]:] = 1.0                  # (one head kept: the second)
        zi[i, torch.randperm(4 * WIDTH, generator=g)[:INTER_KEPT[i]]] = 1.0
    return zh, zd, zi, torch.tensor(FFN_Z)


def toy_tower(hidden_keep=101, act_layer=None):
    """Transformer(128, layers=5, heads=2) on seeded weights, one composed masked forward (the modules record the masks), then
    prune().  -> the pruned tower (CPU, fp32)."""
    import torch
    from cream_amd.tinyclip.model import Transformer
    torch.manual_seed(11)
    tr = Transformer(WIDTH, LAYERS, HEADS) if act_layer is None else Transformer(WIDTH, LAYERS, HEADS, act_layer=act_layer)
    with torch.no_grad():
        for p in tr.parameters():
            if p.dim() == 1:                                 # biases and LayerNorm parameters away from 0 / 1
                p.add_(0.1 * torch.randn_like(p))
    zh, zd, zi, zf = toy_masks(hidden_keep)
    with torch.no_grad():
        tr(torch.randn(2, 5, WIDTH) * zh, hidden_z=zh, heads_z=zd, intermediate_z=zi, ffn_z=zf)
    return tr.prune()


def sub_tower(tr, idx):
    """A tower of the blocks `idx` of `tr` (shared modules)."""
    import torch
    from cream_amd.tinyclip.model import Transformer
    sub = Transformer.__new__(Transformer)
    torch.nn.Module.__init__(sub)
    sub.width, sub.layers, sub.num_heads, sub.head_dim, sub.mlp_ratio = tr.width, len(idx), tr.num_heads, tr.head_dim, tr.mlp_ratio
    sub.resblocks = torch.nn.ModuleList([tr.resblocks[i] for i in idx])
    return sub
