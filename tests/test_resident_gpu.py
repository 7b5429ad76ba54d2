"""GPU: the device-resident training set (tts_king_amd/resident.py, csrc/collate.hip) against the loader route it replaces — every batch
`ResidentStore.batch` gathers is, field by field, the batch `Dataset` + `reprocess` + `DeviceFeeder` upload for the same utterances;
every byte of the packed buffer that is not a row's own data is zero; the dword path and sources beyond 2^31 bytes give the same
bytes; `TrainEngine` replays its graphs on resident batches with the loader route's losses; `train.main` / `train.evaluate` run on it."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.resident_util import FIELDS, feeder_arrays, make_samples, preprocess_config, store_from_samples, write_corpus
from tts_king_amd import dataset as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUCKETS = [(8, 32, 1000), None]
# utterances 0-4: the edge cases (16 phonemes / 64 frames = exact bucket multiples, one past them, 1 phoneme / 1 frame, 40 frames);
# 8-19: one shape bucket (9..15 phonemes -> 16, 33..63 frames -> 64) for the engine test; the rest mixed
LENS = ([(16, 64), (9, 30), (17, 65), (1, 1), (5, 40), (33, 128), (24, 97), (7, 21)] + [(9 + i % 7, 35 + 2 * i) for i in range(12)] +
        [(5 + 3 * i, 11 + 9 * i) for i in range(12)])
TC = {"optimizer": {"batch_size": 2}}


class Corpus:
    def __init__(self, root, samples):
        from tts_king_amd.resident import ResidentStore
        write_corpus(root, samples)
        self.root, self.samples = root, samples
        self.ds = D.Dataset("train.txt", preprocess_config(root), TC, sort=True, drop_last=True)
        self.store = ResidentStore("train.txt", preprocess_config(root), TC, DEV)

    def feeder(self, idx, bucket):
        """The loader route's batch for these utterances: Dataset -> reprocess -> DeviceFeeder."""
        b = D.reprocess([self.ds[i] for i in idx], range(len(idx)))
        got = list(D.DeviceFeeder([b], DEV, bucket=bucket))
        assert len(got) == 1
        return got[0]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    assert 24 <= len(LENS) <= 40
    return Corpus(str(tmp_path_factory.mktemp("resident")), make_samples(LENS, seed=11))


def assert_same_batch(got, want):
    assert len(got) == len(want) == 15
    for i, (g, w) in enumerate(zip(got, want)):
        if torch.is_tensor(w):
            assert torch.is_tensor(g) and g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (i, g, w)
            assert torch.equal(g, w), "field %d differs" % i
        else:
            assert not torch.is_tensor(g) and np.all(np.asarray(g) == np.asarray(w)), (i, g, w)
    assert (got.t_true, got.l_true) == (want.t_true, want.l_true)
    for g, w in ((got.frame_limit, want.frame_limit), (got.phoneme_limit, want.phoneme_limit)):
        assert (g is None) == (w is None)
        if w is not None:
            assert g.dtype == w.dtype and torch.equal(g, w)
    assert got.layout == want.layout and got.packed.numel() == want.packed.numel() and got.packed.dtype == torch.uint8


CASES = {"b1": [1], "b16": list(range(5, 21)), "exact_multiples": [0, 1], "one_past": [2, 0], "one_phoneme_one_frame": [3],
         "one_phoneme_in_a_batch": [4, 3, 7], "repeated": [6, 6, 5], "all": list(range(len(LENS)))}


@pytest.mark.parametrize("bucket", BUCKETS, ids=["bucket", "nobucket"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_batch_equals_feeder(corpus, case, bucket):
    idx = CASES[case]
    got, want = corpus.store.batch(idx, bucket), corpus.feeder(idx, bucket)
    assert_same_batch(got, want)
    if bucket is not None and case == "exact_multiples":
        assert got.t_true is None and got.l_true is None and got.frame_limit is None and got.phoneme_limit is None
        assert all(not isinstance(tag, str) for tag, *_ in got.layout)
    if bucket is not None and case == "one_past":
        assert (got.t_true, got.l_true, got[5], got[8]) == (65, 17, 24, 96) and got.frame_limit.tolist() == [65] and got.phoneme_limit.tolist() == [17, 17]


def test_mel_longer_than_max_seq_len(corpus):
    bucket = (8, 32, 36)               # 40 frames > max_seq_len 36: bucket_plan keeps Tb = t_true
    got, want = corpus.store.batch([4, 1], bucket), corpus.feeder([4, 1], bucket)
    assert int(got[8]) == 40 and got.t_true is None
    assert_same_batch(got, want)


@pytest.mark.parametrize("bucket", BUCKETS, ids=["bucket", "nobucket"])
def test_short_last_batch_of_a_validation_walk(corpus, bucket):
    from tts_king_amd.resident import ResidentLoader
    loader = ResidentLoader(corpus.store, 5, group_size=4, sort=False, drop_last=False, bucket=bucket)
    plan = [ix.tolist() for ix in loader.index_plan()]
    assert [len(p) for p in plan] == [5, 5, 5, 5, 5, 5, 2] and sum(plan, []) == list(range(32))
    batches = list(loader)
    assert len(batches) == 7
    for k in (0, 6):
        assert_same_batch(batches[k], corpus.feeder(plan[k], bucket))


@pytest.mark.parametrize("bucket", BUCKETS, ids=["bucket", "nobucket"])
@pytest.mark.parametrize("variant", ["float64_energy", "nan_cwt", "frame_level"])
def test_field_variants_equal_feeder(tmp_path, variant, bucket):
    lens = [(9, 30), (16, 64), (17, 65), (3, 5), (6, 33), (12, 40)]
    kw = {"float64_energy": {"energy_dtype": np.float64}, "nan_cwt": {"nan_cwt": True}, "frame_level": {"frame_level": True}}[variant]
    c = Corpus(str(tmp_path), make_samples(lens, seed=5, **kw))
    for idx in ([2, 1, 0], [3], [5, 4, 3, 0]):
        got, want = c.store.batch(idx, bucket), c.feeder(idx, bucket)
        assert_same_batch(got, want)
        if variant == "float64_energy":
            assert got[9].dtype == torch.float64 and got[10].dtype == torch.int64
        if variant == "nan_cwt":
            assert not torch.isnan(got[12]).any() and (got[12] == 0).sum() > (want[12].numel() - sum(11 * lens[i][0] for i in idx))
        if variant == "frame_level" and len(idx) > 1:
            assert got[9].shape[1] == got[11].shape[1] == got[6].shape[1] != got[3].shape[1]
    if variant == "nan_cwt":
        assert any(np.isnan(s["pitch_cwt"]).any() for s in c.samples)


def _host_buffer(samples, idx, bucket):
    """The whole packed buffer as the feeder stages it, gaps zero."""
    arrays, *_ = feeder_arrays(D.reprocess(samples, idx), bucket)
    arrays = [(t, np.nan_to_num(a, nan=0.0) if t == 12 else a, s) for t, a, s in arrays]
    layout, total = D.packed_layout(arrays)
    host = np.zeros(total, dtype=np.uint8)
    D.pack_into(host, layout, arrays)
    return torch.from_numpy(host), tuple(layout)


@pytest.mark.parametrize("bucket", BUCKETS, ids=["bucket", "nobucket"])
def test_every_other_byte_is_zero_and_two_builds_are_equal(corpus, bucket):
    for idx in ([2, 0], [3], list(range(5, 21)), [4, 3, 7]):
        want, layout = _host_buffer(corpus.samples, idx, bucket)
        out = torch.full((want.numel(),), 0xFF, dtype=torch.uint8, device=DEV)
        got = corpus.store.batch(idx, bucket, out=out)
        assert got.packed is out and got.layout == layout
        assert torch.equal(out.cpu(), want), "a byte outside the rows' own data is not zero (or a row's data is wrong)"
        again = corpus.store.batch(idx, bucket)
        assert again.packed is not out and torch.equal(again.packed, out)


def test_unaligned_utterance_starts_take_the_dword_path():
    lens = [(7, 3), (5, 9), (3, 2), (11, 13)]
    samples = make_samples(lens, seed=8, energy_dtype=np.float32, nan_cwt=True)
    aligned = store_from_samples(samples, DEV)
    packed4 = store_from_samples(samples, DEV, align=4)                    # back to back: the second utterance starts at element 7
    e = [f for f in packed4.fields if f.index == 9][0]
    assert e.offsets_host[1] == 7 and (e.offsets_host[1] * 4) % 16 != 0
    # ... and the mel one element off a 16-byte boundary, through the flat form
    fields = {k: [np.asarray(s[name]) for s in samples] for k, name in FIELDS.items()}
    mel = np.concatenate([np.zeros(1, np.float32)] + [s["mel"].reshape(-1) for s in samples])
    offs = 1 + 80 * np.concatenate([[0], np.cumsum([t for _, t in lens])[:-1]])
    fields[6] = (torch.from_numpy(mel).to(DEV), offs, [t for _, t in lens], (80,))
    from tts_king_amd.resident import ResidentStore
    shifted = ResidentStore.from_arrays(fields, device=DEV, align=4)
    for bucket in BUCKETS:
        for idx in ([1, 0], [3, 2, 1, 0], [2]):
            want = aligned.batch(idx, bucket)
            for store in (packed4, shifted):
                got = store.batch(idx, bucket)
                assert got.layout == want.layout and torch.equal(got.packed, want.packed)
            assert torch.equal(want.packed.cpu(), _host_buffer(samples, idx, bucket)[0])


def test_offsets_beyond_2_31_bytes():
    from tts_king_amd.resident import ResidentStore
    lens = [(4, 3), (6, 5)]
    samples = make_samples(lens, seed=9)
    far = 2 ** 29 + 16                                                     # elements: byte 2^31 + 64
    flat = torch.empty(far + 5 * 80 + 64, dtype=torch.float32, device=DEV)  # a little over 2 GiB, uninitialised
    try:
        flat[:3 * 80] = torch.from_numpy(samples[0]["mel"].reshape(-1)).to(DEV)
        flat[far:far + 5 * 80] = torch.from_numpy(samples[1]["mel"].reshape(-1)).to(DEV)
        fields = {k: [np.asarray(s[name]) for s in samples] for k, name in FIELDS.items()}
        fields[6] = (flat, [0, far], [3, 5], (80,))
        store = ResidentStore.from_arrays(fields, device=DEV)
        assert store.nbytes > 2 ** 31
        got = store.batch([1, 0])
        want = torch.from_numpy(D.pad_2D([samples[1]["mel"], samples[0]["mel"]]))
        assert got[6].shape == (2, 5, 80) and torch.equal(got[6].cpu(), want)
        assert torch.equal(got.packed.cpu(), _host_buffer(samples, [1, 0], None)[0])
        del store, got
    finally:
        del flat
        torch.cuda.empty_cache()


def test_kernel_refuses_by_return_code():
    from tts_king_amd import lib, ops
    src = torch.arange(64, dtype=torch.float32, device=DEV)
    offsets = torch.tensor([0, 16], dtype=torch.int64, device=DEV)
    lens_host = np.array([3, 5], dtype=np.int32)
    lens = torch.from_numpy(lens_host).to(DEV)
    out = torch.full((256,), 0xFF, dtype=torch.uint8, device=DEV)

    def call(idx, elem_size=4, padded=5, dst_off=0):
        t = (lib.CollateField * 1)()
        t[0].src, t[0].offsets, t[0].lens, t[0].lens_host = src.data_ptr(), offsets.data_ptr(), lens.data_ptr(), lens_host.ctypes.data
        t[0].n_src, t[0].dst_off, t[0].elem_size, t[0].inner, t[0].padded_rows = 64, dst_off, elem_size, 2, padded
        ih = np.array(idx, dtype=np.int32)
        return ops.collate_batch(t, 1, torch.from_numpy(ih).to(DEV), ih, 2, out)

    for idx in ([0, 2], [-1, 0]):
        with pytest.raises(lib.TtskError, match="outside the store"):
            call(idx)
    with pytest.raises(lib.TtskError, match="utterance 1 has 5 rows, the padded length is 4"):
        call([0, 1], padded=4)
    with pytest.raises(lib.TtskError, match="element size 2, must be 4 or 8"):
        call([0, 1], elem_size=2)
    with pytest.raises(lib.TtskError, match="leaves the buffer"):
        call([0, 1], dst_off=192)
    assert bool((out == 0xFF).all()), "a refused call wrote to the batch buffer"
    call([1, 0])
    want = torch.zeros(2, 5, 2)
    want[0] = torch.arange(16, 26).view(5, 2)
    want[1, :3] = torch.arange(0, 6).view(3, 2)
    assert torch.equal(out[:80].view(torch.float32).view(2, 5, 2).cpu(), want) and bool((out[80:] == 0).all())


def _trainer_config(cfg, root, tmp_path):
    c = copy.deepcopy(cfg)                       # tests/test_trainer_gpu.py's configuration
    c.preprocess_config.path.preprocessed_path = root
    c.train_config["optimizer"]["batch_size"] = 2
    c.train_config["optimizer"]["grad_acc_step"] = 1
    c.train_config["path"] = {"ckpt_path": str(tmp_path / "ckpt"), "log_path": str(tmp_path / "log"), "result_path": str(tmp_path / "res")}
    c.train_config["step"].update({"log_step": 2, "val_step": 4, "save_step": 4, "synth_step": 1000, "total_step": 100})
    c.model_config["transformer"]["encoder_layer"] = c.model_config["transformer"]["decoder_layer"] = 1
    c.gpu = DEV
    c.mi355x["loader_workers"] = 0
    return c


def test_engine_steps_equal_the_loader_route(cfg, corpus, tmp_path):
    """Six batches of one shape bucket through two engines built from the same seed, one fed by ResidentLoader, one by the
    DeviceFeeder on the same index lists: the same losses step by step, and the resident batches are replayed (takes_packed)."""
    import train
    from tts_king_amd.engine import TrainEngine
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.resident import ResidentLoader
    c = _trainer_config(cfg, corpus.root, tmp_path)
    bucket = (8, 32, 1000)
    loader = ResidentLoader(corpus.store, 2, group_size=1, sort=True, drop_last=True, sampler=list(range(8, 20)), bucket=bucket)
    plan = [ix.tolist() for ix in loader.index_plan()]
    assert len(plan) == 6
    runs = []
    for resident in (True, False):
        model, opt = train.get_model(c, DEV, train=True)
        eng = TrainEngine(model, opt, c, FastSpeech2Loss(c.preprocess_config, c.model_config))
        feed = loader if resident else (corpus.feeder(ix, bucket) for ix in plan)
        losses = []
        for step, batch in enumerate(feed, 1):
            assert (int(batch[5]), int(batch[8])) == (16, 64)
            losses.append(eng.step(batch, step)[0])
        eng.wait()
        runs.append(([l.cpu().tolist() for l in losses], dict(eng.stats)))
    (res, res_stats), (ldr, ldr_stats) = runs
    print("resident", res_stats, [round(l[0], 5) for l in res], "loader", ldr_stats, [round(l[0], 5) for l in ldr])
    assert len(res) == len(ldr) == 6 and res_stats == ldr_stats and res_stats["replayed"] > 0
    for step, (a, b) in enumerate(zip(res, ldr), 1):
        assert a == b, "step %d: losses differ: resident %s, loader %s" % (step, a, b)


def test_trainer_runs_on_the_resident_route(cfg, corpus, tmp_path):
    import train
    from tts_king_amd import ops
    from tts_king_amd.resident import ResidentStore
    c = _trainer_config(cfg, corpus.root, tmp_path)
    c.mi355x["resident_data"] = True
    ops.LAUNCH_COUNTS = {}
    try:
        model, opt = train.main(c, max_steps=4)
        n_train = ops.LAUNCH_COUNTS.get("collate_batch", 0)
        assert opt.current_step == 4
        ck = torch.load(os.path.join(c.train_config["path"]["ckpt_path"], "4.pth.tar"))
        assert set(ck) == {"model", "embedding", "optimizer"}
        assert n_train >= 4 + 3                       # four steps, and the validation at step 4 walked val.txt's three batches through it
        val = ResidentStore("val.txt", c.preprocess_config, c.train_config, DEV)
        with_store = train.evaluate(model, 4, c, None, "val", None, DEV, store=val)
        assert ops.LAUNCH_COUNTS["collate_batch"] == n_train + 3
        without = train.evaluate(model, 4, c, None, "val", None, DEV)
        assert ops.LAUNCH_COUNTS["collate_batch"] == n_train + 3
    finally:
        ops.LAUNCH_COUNTS = None
    assert with_store == without and with_store.startswith("Validation Step 4,")


def test_trainer_without_the_key_never_collates(cfg, corpus, tmp_path):
    import train
    from tts_king_amd import ops
    c = _trainer_config(cfg, corpus.root, tmp_path)
    assert "resident_data" not in c.mi355x
    ops.LAUNCH_COUNTS = {}
    try:
        model, opt = train.main(c, max_steps=4)
        counts = dict(ops.LAUNCH_COUNTS)
    finally:
        ops.LAUNCH_COUNTS = None
    assert opt.current_step == 4 and os.path.exists(os.path.join(c.train_config["path"]["ckpt_path"], "4.pth.tar"))
    assert "collate_batch" not in counts
