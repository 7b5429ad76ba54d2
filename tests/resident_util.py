"""Shared by tests/test_resident_cpu.py and tests/test_resident_gpu.py: synthetic utterances with chosen lengths, the preprocessed
directory `Dataset` reads, a `ResidentStore` from the same samples, and the arrays the DeviceFeeder stages for a numpy batch."""
import os

import numpy as np

from tts_king_amd import text as T
from tts_king_amd.dataset import _FIELD_DTYPE

FIELDS = {2: "speaker", 3: "text", 6: "mel", 9: "energy", 10: "duration", 11: "pitch_raw", 12: "pitch_cwt", 13: "pitch_mean", 14: "pitch_std"}


def make_samples(lens, seed=0, frame_level=False, energy_dtype=np.float32, nan_cwt=False):
    """One utterance per (L phonemes, T frames) of `lens`, in the layout of tests/test_dataset_cpu.py:synthetic_samples.  Phoneme
    numbers are 150..199, what `text_to_sequence` gives back for the metadata `write_corpus` writes.  frame_level: energy and
    pitch have T entries, not L."""
    rng = np.random.RandomState(seed)
    out = []
    for i, (Ln, Tn) in enumerate(lens):
        dur = np.ones(Ln, dtype=np.int64)
        dur[0] += Tn - Ln                     # (callers give T >= L)
        n = Tn if frame_level else Ln
        cwt = rng.randn(Ln, 11).astype(np.float32)
        if nan_cwt:
            cwt[rng.rand(Ln, 11) < 0.3] = np.nan
        out.append({"id": "utt%03d" % i, "speaker": int(rng.randint(0, 3)), "text": 150 + rng.randint(0, 50, size=Ln), "raw_text": "raw %d" % i,
                    "mel": rng.randn(Tn, 80).astype(np.float32), "energy": rng.randn(n).astype(energy_dtype), "duration": dur,
                    "pitch_raw": rng.randn(n).astype(np.float32), "pitch_mean": np.float32(rng.randn()),
                    "pitch_std": np.float32(abs(rng.randn()) + 0.1), "pitch_cwt": cwt})
    return out


def write_corpus(root, samples, n_val=6):
    """The preprocessed directory of `samples` (tests/test_trainer_gpu.py:write_corpus for given samples): train.txt = all, val.txt =
    the first n_val."""
    for d in ("mel", "energy", "duration", "pitch"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    syms = T.symbols()
    lines = []
    for s in samples:
        spk, b = "spk%d" % s["speaker"], s["id"]
        phon = "{" + " ".join(syms[i][1:] for i in s["text"]) + "}"
        lines.append("%s|%s|%s|%s" % (b, spk, phon, s["raw_text"]))
        for d, kind, key in (("mel", "mel", "mel"), ("energy", "energy", "energy"), ("duration", "duration", "duration"), ("pitch", "pitch", "pitch_raw"),
                             ("pitch", "cwt-pitch", "pitch_cwt"), ("pitch", "pitch-mean", "pitch_mean"), ("pitch", "pitch-std", "pitch_std")):
            np.save(os.path.join(root, d, "%s-%s-%s.npy" % (spk, kind, b)), s[key])
    with open(os.path.join(root, "train.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(root, "val.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines[:n_val]) + "\n")
    with open(os.path.join(root, "speakers.json"), "w") as f:
        f.write('{"spk0": 0, "spk1": 1, "spk2": 2}')
    import shutil
    shutil.copy(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pretrained", "stats.json"), os.path.join(root, "stats.json"))


def preprocess_config(root):
    return {"path": {"preprocessed_path": str(root)}, "preprocessing": {"text": {"text_cleaners": []}}}


def store_from_samples(samples, device, **kw):
    from tts_king_amd.resident import ResidentStore
    return ResidentStore.from_arrays({k: [np.asarray(s[name]) for s in samples] for k, name in FIELDS.items()}, ids=[s["id"] for s in samples],
                                     raw_texts=[s["raw_text"] for s in samples], device=device, **kw)


def feeder_arrays(b, bucket):
    """What DeviceFeeder._preload stages for the numpy 15-tuple `b`: ([(tag, array, target shape)], Lb, Tb, t_true, l_true)."""
    from tts_king_amd.engine import bucket_plan
    axis1, b = {}, list(b)
    t_true = l_true = None
    if bucket is not None:
        Lb, Tb, t_true, l_true, axis1 = bucket_plan(b, *bucket)
        b[5], b[8] = Lb, Tb
    arrays = []
    for i, x in enumerate(b):
        if isinstance(x, np.ndarray) and x.dtype != object:
            a = x.astype(_FIELD_DTYPE[i], copy=False) if i in _FIELD_DTYPE else x
            shp = a.shape if i not in axis1 else (a.shape[0], axis1[i]) + tuple(a.shape[2:])
            arrays.append((i, a, tuple(shp)))
    if t_true is not None:
        arrays.append(("fl", np.array([t_true], dtype=np.int32), (1,)))
    if l_true is not None:
        arrays.append(("pl", np.full((len(b[0]),), l_true, dtype=np.int64), (len(b[0]),)))
    return arrays, b[5], b[8], t_true, l_true
