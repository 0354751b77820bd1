"""Golden files of the saved-logits format, made by the reference's own `TxtManager` (TinyViT/data/augmentation/manager.py,
loaded read-only as a stand-alone module: it imports the standard library only):

    tinyvit_logits/logits_top5_epoch0/rank{0,1}-keys.txt, rank{0,1}-values.bin    what its writer leaves for two ranks; rank 0
                                                                                 is handed one key twice (the first wins)
    tinyvit_logits/readback.json    what its reader returns per key (hex) for rank 0 and rank 1, the records as written
                                    (seed, indices, values) and the order in which each rank's reader lists the packages

Data only.  Run from the repository root with the reference checkout present:  python tests/golden/make_tinyvit_logits_golden.py"""
import importlib.util
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "tinyvit_logits")
TOPK, EPOCH, NUM_CLASSES = 5, 0, 300
ITEM_SIZE = 4 + 4 * TOPK
# (rank, key, seed, indices, values): "n01/b.JPEG" comes twice on rank 0
RECORDS = [
    (0, "n01/a.JPEG", 17, [7, 299, 0, 12, 150], [0.5, 0.25, 0.125, 0.03125, 0.0009765625]),
    (0, "n01/b.JPEG", 2147483647, [1, 2, 3, 4, 5], [0.40625, 0.203125, 0.1015625, 0.05078125, 0.025390625]),
    (0, "n01/b.JPEG", 5, [9, 8, 7, 6, 5], [0.2, 0.2, 0.2, 0.2, 0.1]),
    (0, "n02/c.JPEG", 0, [290, 291, 292, 293, 294], [0.99, 0.004, 0.003, 2e-5, 6e-8]),
    (1, "n02/d.JPEG", 123456789, [100, 50, 25, 12, 6], [0.3, 0.2, 0.1, 0.05, 0.01]),
    (1, "n03/e.JPEG", 1, [0, 1, 2, 3, 4], [0.6, 0.1, 0.1, 0.1, 0.05]),
    (1, "n03/f.JPEG", 99, [11, 22, 33, 44, 55], [0.21, 0.2, 0.19, 0.18, 0.17]),
]


def record_bytes(seed, indices, values):
    return np.int32(seed).tobytes() + np.asarray(indices, np.int16).tobytes() + np.asarray(values, np.float16).tobytes()


def load_manager():
    import refshim
    assert refshim.have_reference(), "needs the reference checkout"
    path = os.path.join(refshim.REFERENCE, "TinyViT", "data", "augmentation", "manager.py")
    spec = importlib.util.spec_from_file_location("ref_tinyvit_manager", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_manager()
    shutil.rmtree(OUT, ignore_errors=True)
    path = os.path.join(OUT, f"logits_top{TOPK}_epoch{EPOCH}")
    for rank in (0, 1):
        manager = ref.TxtManager(path, ITEM_SIZE, rank)
        for r, key, seed, indices, values in RECORDS:
            if r == rank:
                manager.write(key, record_bytes(seed, indices, values))
        manager.writer.__del__()                       # the reference's way to finish: its worker moves the files into `path`
        manager.writer.worker = None
    keys = sorted({key for _, key, *_ in RECORDS})
    out = {"topk": TOPK, "epoch": EPOCH, "num_classes": NUM_CLASSES, "item_size": ITEM_SIZE, "keys": keys,
           "written": [dict(rank=r, key=key, seed=seed, index=indices, value=[float(np.float16(v)) for v in values])
                       for r, key, seed, indices, values in RECORDS]}
    for rank in (0, 1):
        manager = ref.TxtManager(path, ITEM_SIZE, rank)
        out[f"rank{rank}"] = {key: manager.read(key).hex() for key in keys}
        out[f"rank{rank}_packages"] = [os.path.basename(p.name) for p in manager.reader.packages]
    with open(os.path.join(OUT, "readback.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for name in sorted(os.listdir(path)):
        print(name, os.path.getsize(os.path.join(path, name)))


if __name__ == "__main__":
    main()
