"""TinyViT's fast pretraining distillation (TinyViT/save_logits.py, TinyViT/main.py:284-359, TinyViT/data/augmentation/
{dataset_wrapper,manager}.py) on the project's own kernels, with the reference's file format on disk.

A teacher's soft labels are saved ONCE as sparse records — per image an int32 augmentation seed and the top-k softmax
probabilities as int16 index / fp16 value — and the student trains on the records:

    writer side   save_logits_epoch -> topk_records (csrc/sparse_distill.hip: softmax, top-k and the record layout in one
                  launch) -> LogitsWriter ({path}/rank{r}-keys.txt, {path}/rank{r}-values.bin)
    reader side   SeededDeviceBatches (read mode) -> LogitsReader -> distill_step -> sparse_soft_target_cross_entropy
                  (cream_sparse_ce: loss and dense logit gradient from the sparse record; the reference's dense (B, C)
                  teacher tensor is never built)

Left out, as in the issue this module answers: the teacher models, the yacs config and launcher, seeded Mixup / CutMix (the
recipe disables them), gradient accumulation, the reference's writer process."""
import os
import random

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .autoformer import data as _data
from .autoformer.block import _p, _stream

MAX_K, MAX_CLASSES = 128, 32768              # the kernels' range (include/cream_amd.h)


# ---- the loss ---------------------------------------------------------------------------------------------------------
def recover_teacher(index, value, num_classes):
    """main.py:321-328 restated: the dense (B, num_classes) fp32 teacher of a top-k record — `value` at `index`, the rest
    of the probability mass spread evenly over the other classes."""
    index, value = index.long(), value.float()
    minor = (1.0 - value.sum(-1, keepdim=True)) / (num_classes - index.shape[-1])
    return minor.repeat_interleave(num_classes, dim=-1).scatter_(-1, index, value)


def dense_soft_target_cross_entropy(outputs, index, value):
    """The reference's formulation (main.py:321-330 with timm's SoftTargetCrossEntropy; log_softmax in fp32 as under
    autocast): what the kernel replaces and what every unsupported input falls back to."""
    teacher = recover_teacher(index.to(outputs.device), value.to(outputs.device), outputs.shape[-1])
    return torch.sum(-teacher * F.log_softmax(outputs.float(), dim=-1), dim=-1).mean()


def sparse_ce_supported(outputs, index, value):
    if not (outputs.is_cuda and outputs.dim() == 2 and outputs.dtype in (torch.bfloat16, torch.float32)):
        return False
    B, C = outputs.shape
    return (index.dim() == 2 and index.shape == value.shape and index.shape[0] == B and 1 <= index.shape[1] <= MAX_K and
            index.shape[1] < C <= MAX_CLASSES and index.dtype == torch.int16 and value.dtype == torch.float16 and
            index.device == outputs.device and value.device == outputs.device and not value.requires_grad)


class SparseSoftTargetCEFunction(torch.autograd.Function):
    """mean_b of the soft-target cross entropy against the record's dense teacher; loss rows and the logit gradient come
    from the SAME launch (cream_sparse_ce), the gradient is scaled by the incoming one and rounded once to outputs.dtype."""

    @staticmethod
    def forward(ctx, outputs, index, value):
        lib = _lib.load()
        B, C = outputs.shape
        x, idx, val = outputs.contiguous(), index.contiguous(), value.contiguous()
        rows = torch.empty(B, dtype=torch.float32, device=x.device)
        dl = torch.empty((B, C), dtype=torch.float32, device=x.device)
        code = _lib.BF16 if x.dtype == torch.bfloat16 else _lib.F32
        _lib.check(lib.cream_sparse_ce(_p(rows), _p(dl), _p(x), _p(idx), _p(val), B, C, idx.shape[1], code, 1.0 / B, _stream()),
                   "cream_sparse_ce")
        ctx.save_for_backward(dl)
        ctx.out_dtype = outputs.dtype
        return rows.mean()

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        out = torch.empty(dl.shape, dtype=ctx.out_dtype, device=dl.device)
        torch.mul(dl, g, out=out)
        return out, None, None


def sparse_soft_target_cross_entropy(outputs, index, value):
    """criterion(outputs, recover_teacher(index, value)) of the distillation step (main.py:321-330), mean over the batch.
    index (B, k) int16 and value (B, k) fp16 are the record's fields as stored.  Device tensors within the kernel's range:
    one launch; CPU tensors, other dtypes and shapes outside the range: the reference's dense formulation."""
    if sparse_ce_supported(outputs, index, value):
        return SparseSoftTargetCEFunction.apply(outputs, index, value)
    return dense_soft_target_cross_entropy(outputs, index, value)


def accuracy(outputs, target, topk=(1, 5)):
    """timm.utils.accuracy: per cent of rows whose target is among the top-k outputs."""
    maxk = min(max(topk), outputs.shape[1])
    pred = outputs.topk(maxk, 1, True, True)[1].t()
    correct = pred.eq(target.reshape(1, -1).expand_as(pred))
    return [correct[:min(k, maxk)].reshape(-1).float().sum(0) * 100. / target.shape[0] for k in topk]


def teacher_accuracy(index, target):
    """Teacher top-1 / top-5 (main.py:350-351) straight from the record: its indices are sorted largest first, so the dense
    teacher's top-5 are the first five entries."""
    hit = index.long() == target.reshape(-1, 1).long()
    n = target.shape[0]
    return hit[:, :1].any(1).float().sum() * 100. / n, hit[:, :5].any(1).float().sum() * 100. / n


# ---- records ------------------------------------------------------------------------------------------------------------
def item_size(topk):
    """Bytes of one record: the int32 seed, topk int16 indices, topk fp16 values (dataset_wrapper.py:63-64)."""
    return 4 + 4 * topk


def topk_records_supported(outputs, seeds, k):
    return (outputs.is_cuda and outputs.dim() == 2 and outputs.dtype in (torch.bfloat16, torch.float32) and 1 <= k <= MAX_K and
            k <= outputs.shape[1] <= MAX_CLASSES and seeds.dtype == torch.int32 and seeds.device == outputs.device and
            seeds.shape == outputs.shape[:1])


def topk_records_torch(outputs, seeds, k):
    """save_logits.py:135-157 with the framework's operators: softmax (fp32, as under autocast), topk, the two casts and
    the record layout as one (B, 4 + 4k) uint8 tensor."""
    values, indices = torch.softmax(outputs.float(), -1).topk(k=k, dim=-1, largest=True, sorted=True)
    seeds = seeds.to(device=outputs.device, dtype=torch.int32).reshape(-1, 1).contiguous()
    parts = [seeds.view(torch.uint8), indices.to(torch.int16).contiguous().view(torch.uint8),
             values.to(torch.float16).contiguous().view(torch.uint8)]
    return torch.cat(parts, dim=1)


def topk_records(outputs, seeds, k):
    """(B, 4 + 4k) uint8: per row the record `seed | top-k indices | top-k softmax values` of save_logits.py:135-157.
    Device tensors within the kernel's range: one launch (cream_softmax_topk_records; larger logit first, ties by ascending
    class); otherwise softmax, topk and casts of the framework."""
    if not topk_records_supported(outputs, seeds, k):
        return topk_records_torch(outputs, seeds, k)
    lib = _lib.load()
    B, C = outputs.shape
    x, s = outputs.contiguous(), seeds.contiguous()
    rec = torch.empty((B, item_size(k)), dtype=torch.uint8, device=x.device)
    code = _lib.BF16 if x.dtype == torch.bfloat16 else _lib.F32
    _lib.check(lib.cream_softmax_topk_records(_p(rec), _p(x), _p(s), B, C, k, code, _stream()), "cream_softmax_topk_records")
    return rec


def pack_records(seeds, index, value):
    """numpy codec, writer side (save_logits.py:156-157): (B) int32, (B, k) int16, (B, k) fp16 -> (B, 4 + 4k) uint8."""
    seeds = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 1)
    index, value = np.ascontiguousarray(index), np.ascontiguousarray(value)
    if index.dtype != np.int16 or value.dtype != np.float16 or index.shape != value.shape or index.ndim != 2 or len(index) != len(seeds):
        raise ValueError("pack_records takes (B) int32 seeds, (B, k) int16 indices and (B, k) float16 values")
    return np.concatenate([seeds.view(np.uint8), index.view(np.uint8), value.view(np.uint8)], axis=1)


def unpack_records(records, topk, num_classes):
    """numpy codec, reader side (dataset_wrapper.py:47-60): one record (bytes) or a (B, 4 + 4 topk) uint8 array ->
    (seeds (B) int32, index (B, topk) int16, value (B, topk) fp16).  Raises ValueError on a wrong item size, an index outside
    [0, num_classes) or an index repeated within a row — records the loss kernel's contract excludes."""
    if isinstance(records, (bytes, bytearray, memoryview)):
        records = np.frombuffer(bytes(records), dtype=np.uint8).reshape(1, -1)
    records = np.ascontiguousarray(records, dtype=np.uint8)
    if records.ndim != 2 or records.shape[1] != item_size(topk):
        raise ValueError(f"a record of top-{topk} logits has {item_size(topk)} bytes, got an array of shape {records.shape}")
    seeds = records[:, :4].copy().view(np.int32).reshape(-1)
    index = records[:, 4:4 + 2 * topk].copy().view(np.int16)
    value = records[:, 4 + 2 * topk:].copy().view(np.float16)
    if index.size and (index.min() < 0 or index.max() >= num_classes):
        raise ValueError(f"record index outside [0, {num_classes})")
    srt = np.sort(index, axis=1)
    if topk > 1 and bool((srt[:, 1:] == srt[:, :-1]).any()):
        raise ValueError("record with a repeated class index")
    return seeds, index, value


# ---- the on-disk format (manager.py) ------------------------------------------------------------------------------------
def logits_dir(root, topk, epoch):
    """dataset_wrapper.py:75-76."""
    return os.path.join(root, f"logits_top{topk}_epoch{epoch}")


class LogitsWriter:
    """One rank's package of an epoch directory: `{path}/rank{r}-keys.txt` (one key per line) and `{path}/rank{r}-values.bin`
    (fixed-size items in key order) — the files of the reference's TxtManager writer.  The first record of a repeated key is
    kept.  Synchronous: the files grow under temporary names and are renamed on close() (the reference's worker process and
    its shell `mv` are not reproduced)."""

    def __init__(self, path, rank=0):
        self.path, self.rank = path, rank
        os.makedirs(path, exist_ok=True)
        stem = os.path.join(path, f"rank{rank}")
        self._final = (stem + "-keys.txt", stem + "-values.bin")
        self._tmp = tuple(f + ".tmp" for f in self._final)
        self._keys_file = open(self._tmp[0], "w")
        self._values_file = open(self._tmp[1], "wb")
        self._keys = set()

    def write(self, key, value):
        if self._keys_file is None:
            raise ValueError("write to a closed LogitsWriter")
        if key in self._keys:
            return False
        self._keys.add(key)
        self._keys_file.write(key + "\n")
        self._values_file.write(bytes(value))
        return True

    def close(self):
        if self._keys_file is None:
            return
        self._keys_file.close()
        self._values_file.close()
        self._keys_file = self._values_file = None
        for tmp, final in zip(self._tmp, self._final):
            os.replace(tmp, final)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class LogitsReader:
    """Reads records by key from every package of an epoch directory, as the reference's TxtManager reader does: packages
    are visited in the order (r - rank) mod n (a rank finds its own keys first), a package's key file is loaded only when a
    key is not known yet, and its values file is opened at the first read from it."""

    def __init__(self, path, topk, rank=0):
        if not os.path.isdir(path):
            raise FileNotFoundError(f"no saved logits at {path}")
        self.path, self.topk, self.rank, self.item_size = path, topk, rank, item_size(topk)
        suffix = "-values.bin"
        names = [n[:-len(suffix)] for n in os.listdir(path) if n.endswith(suffix)]
        count = len(names)
        names.sort(key=lambda n: (int(n[4:]) - rank) % count)
        self._packages = [os.path.join(path, n) for n in names]
        self._visited = 0                      # packages whose key files are loaded
        self._handles = [None] * len(names)
        self._where = {}                       # key -> (package, item)

    def _find(self, key):
        while key not in self._where and self._visited < len(self._packages):
            p = self._visited
            self._visited += 1
            with open(self._packages[p] + "-keys.txt") as fh:
                for i, line in enumerate(fh.readlines()):
                    self._where[line.strip()] = (p, i)         # a later package's copy of a key replaces an earlier one
        return self._where[key]

    def read(self, key):
        """The record's bytes.  KeyError for a key no package holds."""
        p, i = self._where[key] if key in self._where else self._find(key)
        if self._handles[p] is None:
            self._handles[p] = open(self._packages[p] + "-values.bin", "rb")
        self._handles[p].seek(self.item_size * i)
        return self._handles[p].read(self.item_size)

    def close(self):
        for h in self._handles:
            if h is not None:
                h.close()
        self._handles = [None] * len(self._handles)


# ---- seeded input batches -------------------------------------------------------------------------------------------------
class SeededDeviceBatches(_data.DeviceBatches):
    """DeviceBatches whose training augmentation of every image is a function of one int32 seed, so that the student sees
    exactly the crop the teacher labelled (dataset_wrapper.py:32-45).  `loader` yields (frames, labels, keys).

    write mode (`reader` None): draws one seed per image as dataset_wrapper.py:35 does (`seed_rng.randint(0, 1 << 31)`,
        numpy's global generator by default) and yields (samples, labels, keys, seeds);
    read mode (`reader` a LogitsReader): looks the record up by key, replays the parameters from the stored seed and yields
        (samples, labels, index (B, k) int16, value (B, k) fp16, seeds) — tensors on the device, seeds int32.

    The FORMAT of the records is the reference's; the DRAW STREAM is this project's: crop, flip, RandAugment and erase
    parameters come from `random.Random(seed)` and `np.random.RandomState(seed)` in DeviceBatches' order of draws, while
    the reference routes a PCG64 generator through its own forks of the timm transforms.  Records written by the reference
    therefore pair with the reference's augmentations, not with these."""

    def __init__(self, loader, transform, reader=None, num_classes=None, reprob=0.0, auto_augment=None, seed_rng=None):
        super().__init__(loader, transform, mode="train", reprob=reprob, auto_augment=auto_augment)
        self.reader, self.num_classes = reader, num_classes
        self.seed_rng = seed_rng if seed_rng is not None else np.random
        if reader is not None and num_classes is None:
            raise ValueError("read mode needs num_classes (records are validated against it)")

    def draw_seeds(self, n):
        return np.array([np.int32(self.seed_rng.randint(0, 1 << 31)) for _ in range(n)], dtype=np.int32)

    def params_for(self, shapes, seeds):
        """DeviceBatches.params_for in training mode, image i drawing from generators seeded with seeds[i] alone."""
        out = []
        for shape, seed in zip(shapes, seeds):
            self.rng, self.np_rng = random.Random(int(seed)), np.random.RandomState(int(seed))
            out.extend(super().params_for([shape]))
        return out

    def _samples(self, frames, seeds):
        params = self.params_for([tuple(f.shape[:2]) for f in frames], seeds)
        if self.auto_augment is not None:
            return self.transform(frames, [p[:5] for p in params], aug_ops=[p[5] for p in params])
        return self.transform(frames, params)

    def __iter__(self):
        for frames, labels, keys in self.loader:
            if self.reader is None:
                seeds = self.draw_seeds(len(frames))
            else:
                raw = np.frombuffer(b"".join(self.reader.read(k) for k in keys), dtype=np.uint8)
                seeds, index, value = unpack_records(raw.reshape(len(keys), -1), self.reader.topk, self.num_classes)
            samples = self._samples(frames, seeds)
            dev = samples.device
            labels = torch.as_tensor(labels, dtype=torch.int64).to(dev, non_blocking=True)
            seeds_t = torch.from_numpy(seeds).to(dev, non_blocking=True)
            if self.reader is None:
                yield samples, labels, list(keys), seeds_t
            else:
                yield samples, labels, torch.from_numpy(index).to(dev), torch.from_numpy(value).to(dev), seeds_t


# ---- drivers ----------------------------------------------------------------------------------------------------------------
def _autocast(device):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=device.type == "cuda")


@torch.no_grad()
def save_logits_epoch(teacher, batches, writer, k):
    """save_logits.py:102-160: the teacher in eval mode under bf16 autocast over one epoch of write-mode batches; every image's
    record goes to `writer` under its key.  -> {'teacher_acc1', 'teacher_acc5', 'images'} (batch-size weighted means)."""
    teacher.eval()
    n, a1, a5 = 0, 0.0, 0.0
    for samples, labels, keys, seeds in batches:
        with _autocast(samples.device):
            outputs = teacher(samples)
        acc1, acc5 = accuracy(outputs, labels)
        records = topk_records(outputs, seeds, k).cpu().numpy()
        for key, rec in zip(keys, records):
            writer.write(key, rec.tobytes())
        b = len(keys)
        n, a1, a5 = n + b, a1 + float(acc1) * b, a5 + float(acc5) * b
    return {"teacher_acc1": a1 / max(n, 1), "teacher_acc5": a5 / max(n, 1), "images": n}


def distill_step(model, optimizer, batch, max_norm=None, criterion=sparse_soft_target_cross_entropy):
    """One step of main.py:303-353 on a read-mode batch (samples, labels, index, value, seeds): forward under bf16 autocast,
    the sparse soft-target loss, backward, the optimizer step — `NativeAdamW.step(max_norm=...)` clips inside its launch, any
    other optimizer gets torch's clip_grad_norm_ first.  -> the meters the reference logs, as floats."""
    from .autoformer.engine import NativeAdamW
    samples, labels, index, value, _ = batch
    model.train()
    optimizer.zero_grad(set_to_none=not isinstance(optimizer, NativeAdamW))     # NativeAdamW's job table holds the gradient tensors
    with _autocast(samples.device):
        outputs = model(samples)
    loss = criterion(outputs, index, value)
    loss.backward()
    if isinstance(optimizer, NativeAdamW):
        optimizer.step(max_norm=max_norm)
    else:
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        optimizer.step()
    acc1, acc5 = accuracy(outputs.detach(), labels)
    t1, t5 = teacher_accuracy(index, labels)
    return {"loss": float(loss.detach()), "train_acc1": float(acc1), "train_acc5": float(acc5), "teacher_acc1": float(t1),
            "teacher_acc5": float(t5)}
