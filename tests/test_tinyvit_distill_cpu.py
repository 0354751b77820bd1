"""cream_amd/tinyvit_distill.py without a device: the record codec, the on-disk format against files written and read back by
the reference's own TxtManager (tests/golden/make_tinyvit_logits_golden.py), the seeded replay of augmentation parameters and
the teacher meters."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tinyvit_logits")


def _T():
    from cream_amd import tinyvit_distill as T
    return T


def _fixture():
    with open(os.path.join(GOLDEN, "readback.json")) as fh:
        return json.load(fh)


def _records(B=4, k=5, C=300, seed=0):
    rng = np.random.RandomState(seed)
    seeds = rng.randint(0, 1 << 31, B).astype(np.int32)
    index = np.stack([rng.permutation(C)[:k] for _ in range(B)]).astype(np.int16)
    value = np.sort(rng.rand(B, k), axis=1)[:, ::-1].astype(np.float16) / k
    return seeds, index, value


def test_codec_round_trip():
    T = _T()
    seeds, index, value = _records()
    rec = T.pack_records(seeds, index, value)
    assert rec.dtype == np.uint8 and rec.shape == (4, T.item_size(5)) and T.item_size(100) == 404
    for row, s, i, v in zip(rec, seeds, index, value):
        assert row.tobytes() == s.tobytes() + i.tobytes() + v.tobytes()
    s2, i2, v2 = T.unpack_records(rec, 5, 300)
    assert np.array_equal(s2, seeds) and np.array_equal(i2, index) and np.array_equal(v2.view(np.uint16), value.view(np.uint16))
    s1, i1, v1 = T.unpack_records(rec[2].tobytes(), 5, 300)                     # one record as bytes, as a reader returns it
    assert s1[0] == seeds[2] and np.array_equal(i1[0], index[2]) and np.array_equal(v1[0], value[2])


def test_unpack_rejects_malformed_records():
    T = _T()
    seeds, index, value = _records()
    rec = T.pack_records(seeds, index, value)
    with pytest.raises(ValueError, match="bytes"):
        T.unpack_records(rec, 6, 300)                                           # wrong item size
    with pytest.raises(ValueError, match="bytes"):
        T.unpack_records(rec[0].tobytes()[:-1], 5, 300)
    for bad in (300, -1):
        idx = index.copy()
        idx[1, 3] = bad
        with pytest.raises(ValueError, match="outside"):
            T.unpack_records(T.pack_records(seeds, idx, value), 5, 300)         # index outside [0, num_classes)
    idx = index.copy()
    idx[3, 4] = idx[3, 0]
    with pytest.raises(ValueError, match="repeated"):
        T.unpack_records(T.pack_records(seeds, idx, value), 5, 300)             # the same class twice in a row


@pytest.mark.parametrize("rank", [0, 1])
def test_reader_returns_what_the_reference_reader_returned(rank):
    T, fix = _T(), _fixture()
    path = T.logits_dir(GOLDEN, fix["topk"], fix["epoch"])
    assert os.path.basename(path) == "logits_top5_epoch0"
    reader = T.LogitsReader(path, fix["topk"], rank)
    assert [os.path.basename(p) for p in reader._packages] == fix[f"rank{rank}_packages"]
    assert reader._handles == [None, None] and reader._visited == 0            # nothing is opened before the first read
    for key in fix["keys"]:
        assert reader.read(key).hex() == fix[f"rank{rank}"][key], key
    own = [w["key"] for w in fix["written"] if w["rank"] == rank][0]
    fresh = T.LogitsReader(path, fix["topk"], rank)
    fresh.read(own)
    assert fresh._visited == 1 and fresh._handles[1] is None                    # a rank's own keys need its own package only
    with pytest.raises(KeyError):
        reader.read("n09/missing.JPEG")
    # the records decode to what the maker wrote; the repeated key kept its first record
    first = {}
    for w in fix["written"]:
        first.setdefault(w["key"], w)
    for key, w in first.items():
        seed, index, value = T.unpack_records(reader.read(key), fix["topk"], fix["num_classes"])
        assert seed[0] == w["seed"] and index[0].tolist() == w["index"] and value[0].astype(np.float64).tolist() == w["value"]
    reader.close()
    fresh.close()


def test_writer_output_is_byte_identical_to_the_reference_writers(tmp_path):
    T, fix = _T(), _fixture()
    path = T.logits_dir(str(tmp_path), fix["topk"], fix["epoch"])
    for rank in (0, 1):
        with T.LogitsWriter(path, rank) as writer:
            kept = [writer.write(w["key"], T.pack_records([w["seed"]], np.array([w["index"]], np.int16),
                                                          np.array([w["value"]], np.float16))[0].tobytes())
                    for w in fix["written"] if w["rank"] == rank]
            assert not any(n.endswith(("-keys.txt", "-values.bin")) for n in os.listdir(path) if n.startswith(f"rank{rank}"))
        assert kept == ([True, True, False, True] if rank == 0 else [True, True, True])
    ref_dir = T.logits_dir(GOLDEN, fix["topk"], fix["epoch"])
    assert sorted(os.listdir(path)) == sorted(os.listdir(ref_dir)) == ["rank0-keys.txt", "rank0-values.bin", "rank1-keys.txt",
                                                                      "rank1-values.bin"]
    for name in os.listdir(ref_dir):
        with open(os.path.join(path, name), "rb") as a, open(os.path.join(ref_dir, name), "rb") as b:
            assert a.read() == b.read(), name


class _Size:
    size = 64
    mean = (0.485, 0.456, 0.406)


def test_seeded_params_replay_from_the_stored_seeds():
    """params_for is a function of (shape, seed) alone: write mode and the replay from the stored seeds agree, whatever was
    drawn in between, and different seeds give different crops."""
    T = _T()
    shapes = [(75, 100), (90, 60), (64, 64), (120, 80)]
    write = T.SeededDeviceBatches([], _Size(), reprob=0.25, auto_augment="rand-m9-mstd0.5-inc1", seed_rng=np.random.RandomState(3))
    seeds = write.draw_seeds(len(shapes))
    assert seeds.dtype == np.int32 and (seeds >= 0).all() and len(set(seeds.tolist())) == len(shapes)
    again = np.random.RandomState(3)
    assert seeds.tolist() == [int(np.int32(again.randint(0, 1 << 31))) for _ in shapes]      # dataset_wrapper.py:35, per image
    p_write = write.params_for(shapes, seeds)
    write.params_for(shapes[::-1], seeds + 1)                                                   # unrelated draws in between
    read = T.SeededDeviceBatches([], _Size(), reprob=0.25, auto_augment="rand-m9-mstd0.5-inc1")
    p_read = read.params_for(shapes, seeds.copy())
    assert repr(p_write) == repr(p_read) and len(p_read) == len(shapes) and all(len(p) == 6 for p in p_read)
    assert repr(read.params_for(shapes[:1], seeds[1:2])) != repr(p_read[:1])
    plain = T.SeededDeviceBatches([], _Size())
    assert repr(plain.params_for(shapes, seeds)) == repr(plain.params_for(shapes, seeds)) and len(plain.params_for(shapes, seeds)[0]) == 5
    with pytest.raises(ValueError):
        T.SeededDeviceBatches([], _Size(), reader=object())                                     # read mode validates against num_classes


def test_teacher_accuracy_agrees_with_accuracy_over_the_dense_teacher():
    T = _T()
    B, C, k = 64, 300, 10
    g = torch.Generator().manual_seed(0)
    probs = torch.softmax(torch.randn(B, C, generator=g) * 3, -1)
    value, index = probs.topk(k, dim=-1)
    index, value = index.to(torch.int16), value.to(torch.float16)
    target = index[:, 0].long().clone()
    target[::3] = index[::3, 3].long()                       # in the top 5, not first
    target[1::4] = (index[1::4, 9].long())                   # in the record, outside the top 5
    a1, a5 = T.teacher_accuracy(index, target)
    d1, d5 = T.accuracy(T.recover_teacher(index, value, C), target, topk=(1, 5))
    assert float(a1) == float(d1) and float(a5) == float(d5) and 0 < float(a1) < float(a5) < 100
