"""CPU: the host side of the device-resident training set (tts_king_amd/resident.py) — batch order against `dataset.collate` and the
reference's own batches (tests/golden/collate.npz), a batch's shapes and packed layout against `engine.bucket_plan` +
`dataset.packed_layout` on the numpy batch, and what the store refuses.  Stores live on "cpu" here: nothing is gathered."""
import os

import numpy as np
import pytest

from tests.oracle_util import GOLDEN
from tests.resident_util import feeder_arrays, make_samples, preprocess_config, store_from_samples, write_corpus
from tests.test_dataset_cpu import synthetic_samples
from tts_king_amd import dataset as D
from tts_king_amd.resident import ResidentLoader, ResidentStore, index_plan


def _store(samples):
    from tests.resident_util import FIELDS
    return ResidentStore.from_arrays({k: [np.asarray(s[name]) for s in samples] for k, name in FIELDS.items()}, ids=[s["id"] for s in samples],
                                     device="cpu")


def test_batch_order_matches_collate_and_reference():
    g = np.load(os.path.join(GOLDEN, "collate.npz"))
    for tag, (n, bs, sort, drop) in {"a": (11, 4, True, True), "b": (11, 4, True, False), "c": (8, 4, False, True)}.items():
        samples = synthetic_samples(n, 77)
        store = _store(samples)
        plan = ResidentLoader(store, bs, group_size=3, sort=sort, drop_last=drop).index_plan()     # one group of 12 >= n, as collate sees it
        want = D.collate(samples, bs, sort, drop)
        assert len(plan) == len(want) == int(g[tag + "/n"])
        for bi, ix in enumerate(plan):
            ids = [store.ids[i] for i in ix]
            assert ids == list(want[bi][0]) == list(g["%s/%d/ids" % (tag, bi)]), (tag, bi)


def test_batch_order_groups_and_ties():
    # ties keep the sampler's order (stable), groups are sorted one by one, a short last group is cut like any other
    lens = np.array([5, 7, 5, 7, 5, 7, 5, 5])
    assert [ix.tolist() for ix in index_plan(range(8), lens, 2, group_size=4)] == [[1, 3], [5, 0], [2, 4], [6, 7]]
    assert [ix.tolist() for ix in index_plan(range(8), lens, 2, group_size=2)] == [[1, 3], [0, 2], [5, 4], [6, 7]]
    order = [7, 6, 5, 4, 3, 2, 1, 0]
    assert [ix.tolist() for ix in index_plan(order, lens, 3, group_size=2, drop_last=True)] == [[5, 3, 7], [6, 4, 2]]
    assert [ix.tolist() for ix in index_plan(order, lens, 3, group_size=2, drop_last=False)] == [[5, 3, 7], [6, 4, 2], [1, 0]]
    # a group larger than numpy's insertion-sort threshold, half of it tied: still the stable order
    rng = np.random.RandomState(3)
    big = rng.randint(10, 14, size=64)
    order = rng.permutation(64)
    got = np.concatenate(index_plan(order, big, 16, group_size=4))
    assert got.tolist() == sorted(order.tolist(), key=lambda i: -big[i])
    # without ties the order is collate's on the same group of samples (ids in collate's order)
    distinct = [9, 3, 12, 7, 5, 11, 4, 8]
    samples = make_samples([(l, l + 3) for l in distinct], seed=1)
    assert [[samples[i]["id"] for i in ix] for ix in index_plan(range(8), distinct, 4, group_size=2)] == [list(b[0]) for b in D.collate(samples, 4)]


@pytest.mark.parametrize("bucket", [None, (8, 32, 1000), (1, 32, 1000), (8, 32, 36)])
def test_shapes_and_layout_match_bucket_plan(bucket):
    phon = make_samples([(9, 30), (16, 64), (17, 65), (1, 1), (5, 40), (12, 33)], seed=2)
    frame = make_samples([(9, 30), (16, 64), (17, 65), (1, 1), (5, 40), (12, 33)], seed=2, frame_level=True)
    for samples in (phon, frame):
        store = _store(samples)
        for idx in ([0], [1, 0], [2, 1, 0], [3], [4, 0, 3], [0, 1, 2, 3, 4, 5], [5, 5]):
            b = D.reprocess(samples, idx)
            arrays, Lb, Tb, t_true, l_true = feeder_arrays(b, bucket)
            layout, total = D.packed_layout(arrays)
            i32, shapes, got_layout, got_total, gLb, gTb, gt, gl = store.plan(idx, bucket)
            assert i32.dtype == np.int32 and i32.tolist() == idx
            assert (int(gLb), int(gTb), gt, gl) == (int(Lb), int(Tb), t_true, l_true), (idx, bucket)
            assert got_layout == tuple(layout) and got_total == total, (idx, bucket)
            assert shapes == {tag: shp for tag, _, shp in arrays if not isinstance(tag, str)}
    # the frame-level batch really is one: energy and pitch as wide as the mel
    assert store.plan([2, 1], (8, 32, 1000))[1][9] == (2, 96) and store.plan([2, 1], (8, 32, 1000))[1][11] == (2, 96)


def test_store_from_files_equals_store_from_arrays(tmp_path):
    samples = make_samples([(9, 30), (16, 64), (3, 5)], seed=4)
    write_corpus(str(tmp_path), samples, n_val=2)
    a = ResidentStore("train.txt", preprocess_config(tmp_path), {"optimizer": {"batch_size": 2}}, "cpu")
    b = _store(samples)
    assert len(a) == 3 and a.ids == b.ids and a.raw_texts == [s["raw_text"] for s in samples]
    assert a.nbytes == b.nbytes > 3 * 5 * 80 * 4
    for fa, fb in zip(a.fields, b.fields):
        assert fa.index == fb.index and fa.dtype == fb.dtype and fa.tail == fb.tail and fa.flat.equal(fb.flat), fa.index
        assert np.array_equal(fa.offsets_host, fb.offsets_host) and np.array_equal(fa.lens_host, fb.lens_host)
        if fa.index not in (4, 7):            # (the two length fields are the host's length arrays themselves, dense)
            assert not np.any(fa.offsets_host * fa.dtype.itemsize % 16)       # every utterance of a loaded field starts 16-byte aligned
    assert len(ResidentStore("val.txt", preprocess_config(tmp_path), {"optimizer": {"batch_size": 2}}, "cpu")) == 2


def test_refuses_mixed_dtypes_by_field_and_file(tmp_path):
    samples = make_samples([(9, 30), (16, 64), (3, 5)], seed=4)
    samples[2]["energy"] = samples[2]["energy"].astype(np.float64)
    write_corpus(str(tmp_path), samples)
    with pytest.raises(ValueError, match=r"energy.*spk\d-energy-utt000\.npy is float32.*spk\d-energy-utt002\.npy is float64"):
        ResidentStore("train.txt", preprocess_config(tmp_path), {"optimizer": {"batch_size": 2}}, "cpu")
    with pytest.raises(ValueError, match="energy.*mixed dtypes"):
        _store(samples)


def test_refuses_store_over_resident_max_gb():
    samples = make_samples([(9, 30), (16, 64)], seed=4)
    with pytest.raises(MemoryError, match=r"GB.*mi355x\.resident_max_gb = 1e-05"):
        store_from_samples(samples, "cpu", max_gb=1e-5)
    assert len(store_from_samples(samples, "cpu", max_gb=1e-3)) == 2


def test_refuses_index_outside_store():
    store = _store(make_samples([(9, 30), (16, 64)], seed=4))
    for bad in ([0, 2], [-1], []):
        with pytest.raises(IndexError, match="outside the resident store's 2 utterances"):
            store.plan(bad)
