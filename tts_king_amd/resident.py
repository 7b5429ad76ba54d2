"""The FS2 training set resident on the device, batches collated there (opt-in: `mi355x.resident_data`).

reference: fs_two/dataset.py:32-225 and train.py:83-99 — the same utterances, the same 15-tuple, the same batch order (groups of
batch_size*group_size utterances sorted by phoneme count and cut into batches), but nothing of it per step on the host: `ResidentStore`
reads every utterance's files ONCE (through `Dataset._load` / `text_to_sequence`), keeps each field as one flat device array with a
per-utterance offset and length table, and `ResidentStore.batch` builds a batch with one launch of `ttsk_collate_batch`
(csrc/collate.hip) that writes straight into the packed layout the DeviceFeeder uploads (`dataset.packed_layout`): `TrainEngine`
and `GraphedTrainStep.takes_packed` take it unchanged.  `ResidentLoader` is the DataLoader + collate_fn + DeviceFeeder chain over
index arrays: one small upload of the epoch's index plan, then no host-to-device copy at all.

Host side of a batch (shapes, bucket, layout) comes from the lengths kept in numpy and from `engine.bucket_plan` /
`dataset.packed_layout` themselves, called on arrays that have the batch's shapes and no data.
"""
import numpy as np
import torch

from . import lib as L
from . import ops
from .dataset import _FIELD_DTYPE, Dataset, packed_layout, views_of
from .text import text_to_sequence

ALIGN = 16                          # bytes: every utterance of every field starts on a 16-byte boundary (the kernel's 16-byte loads)
# batch-tuple index -> (directory, file kind) of Dataset._load; name in messages
FILES = {6: ("mel", "mel"), 9: ("energy", "energy"), 10: ("duration", "duration"), 11: ("pitch", "pitch"), 12: ("pitch", "cwt-pitch"),
         13: ("pitch", "pitch-mean"), 14: ("pitch", "pitch-std")}
NAMES = {2: "speaker", 3: "text", 4: "text_lens", 6: "mel", 7: "mel_lens", 9: "energy", 10: "duration", 11: "pitch_raw", 12: "pitch_cwt",
         13: "pitch_mean", 14: "pitch_std"}
SCALARS = (2, 13, 14)               # one value per utterance: gathered like a ragged field whose every length is 1
NAN_TO_ZERO = (12,)                 # as the DeviceFeeder's np.nan_to_num of pitches_cwt


class _Field:
    """One field on the device: `flat` (1-D, every utterance's rows back to back), `offsets` (int64 elements) / `lens` (int32 rows) per
    utterance, `lens_host` the same lengths in numpy, `tail` the shape of one row (() for scalars), `inner` its element count."""

    def __init__(self, index, flat, offsets, lens_host, tail, scalar, device):
        self.index, self.tail, self.scalar = index, tuple(int(t) for t in tail), scalar
        self.inner = int(np.prod(self.tail)) if self.tail else 1
        self.flat = flat if torch.is_tensor(flat) else torch.from_numpy(np.ascontiguousarray(flat)).to(device)
        self.flat = self.flat.reshape(-1)
        self.dtype = np.dtype(str(self.flat.dtype).replace("torch.", ""))
        self.lens_host = np.ascontiguousarray(lens_host, dtype=np.int32)
        self.offsets_host = np.ascontiguousarray(offsets, dtype=np.int64)
        self.offsets = torch.from_numpy(self.offsets_host).to(device)
        self.lens = torch.from_numpy(self.lens_host).to(device)
        if self.dtype.itemsize not in (4, 8):
            raise ValueError("field %s: %s elements; the collate kernel moves 4- and 8-byte elements" % (NAMES.get(index, index), self.dtype))

    @property
    def nbytes(self):
        return self.flat.numel() * self.dtype.itemsize + self.offsets_host.nbytes + self.lens_host.nbytes


def _one_dtype(index, arrays, labels):
    """The arrays' common dtype; ValueError naming the field and the first two that differ."""
    for a, lab in zip(arrays, labels):
        if a.dtype != arrays[0].dtype:
            raise ValueError("field %s: mixed dtypes: %s is %s, %s is %s" % (NAMES.get(index, index), labels[0], arrays[0].dtype, lab, a.dtype))
    return arrays[0].dtype


def _flatten(index, arrays, labels, align=ALIGN):
    """Per-utterance arrays of one field -> (flat 1-D array in the dtype the feeder would upload, offsets in elements, lens in rows,
    row shape).  Utterances start on `align`-byte boundaries (the gaps are zeros and never read)."""
    arrays = [np.asarray(a) for a in arrays]
    _one_dtype(index, arrays, labels)
    dt = np.dtype(_FIELD_DTYPE[index]) if index in _FIELD_DTYPE else arrays[0].dtype
    scalar = index in SCALARS
    tail = arrays[0].shape if scalar else arrays[0].shape[1:]
    for a, lab in zip(arrays, labels):
        if (a.shape if scalar else a.shape[1:]) != tail:
            raise ValueError("field %s: %s has rows of shape %s, %s of shape %s" % (NAMES.get(index, index), labels[0], tail, lab,
                                                                                      a.shape if scalar else a.shape[1:]))
    inner = int(np.prod(tail)) if tail else 1
    lens = np.array([1 if scalar else a.shape[0] for a in arrays], dtype=np.int64)
    step = max(int(align) // dt.itemsize, 1)
    sizes = (lens * inner + step - 1) // step * step
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    flat = np.zeros(int(sizes.sum()), dtype=dt)
    for a, o, n in zip(arrays, offsets, lens * inner):
        flat[o:o + n] = a.reshape(-1)           # (the assignment converts to the feeder's dtype, as its astype does)
    return flat, offsets, lens, tail, scalar


def index_plan(order, text_lens, batch_size, group_size=4, sort=True, drop_last=True):
    """`dataset.collate` over index arrays (reference: train.py:91-99, fs_two/dataset.py:206-225): `order` (a sampler's utterance
    numbers) cut into groups of batch_size*group_size; each group in stable descending order of phoneme count; each group cut into
    batches of batch_size, its remainder kept only when drop_last is False.  Returns a list of int64 index arrays."""
    order = np.asarray(list(order), dtype=np.int64)
    text_lens = np.asarray(text_lens)
    per_group = batch_size * group_size
    out = []
    for g0 in range(0, len(order), per_group):
        grp = order[g0:g0 + per_group]
        n = len(grp)
        k = np.argsort(-text_lens[grp].astype(np.int64), kind="stable") if sort else np.arange(n)
        full = n - n % batch_size
        out += [grp[k[i:i + batch_size]] for i in range(0, full, batch_size)]
        if not drop_last and n % batch_size:
            out.append(grp[k[full:]])
    return out


class ResidentStore:
    """A metadata file's utterances (train.txt / val.txt), every field flat on `device`.  `len(store)` utterances; `nbytes` on the device;
    `text_lens` / `mel_lens` (numpy) are what `reprocess` would compute.  Build with `ResidentStore(filename, preprocess_config,
    train_config, device)` from a preprocessed directory or `ResidentStore.from_arrays(...)` from memory."""

    def __init__(self, filename, preprocess_config, train_config, device, max_gb=32.0):
        ds = Dataset(filename, preprocess_config, train_config)
        n = len(ds)
        path = lambda i, k: "%s/%s-%s-%s.npy" % (FILES[k][0], ds.speaker[i], FILES[k][1], ds.basename[i])
        per = {k: [ds._load(FILES[k][0], FILES[k][1], ds.speaker[i], ds.basename[i]) for i in range(n)] for k in FILES}
        per[2] = [np.array(ds.speaker_map[s]) for s in ds.speaker]
        per[3] = [np.array(text_to_sequence(t, ds.cleaners)) for t in ds.text]
        labels = {k: [path(i, k) for i in range(n)] if k in FILES else list(ds.basename) for k in per}
        self._build({k: _flatten(k, per[k], labels[k]) for k in sorted(per)}, list(ds.basename), list(ds.raw_text), device, max_gb)

    @classmethod
    def from_arrays(cls, fields, ids=None, raw_texts=None, device="cuda:0", max_gb=32.0, align=ALIGN):
        """fields: {batch-tuple index: value} for the indices of `NAMES` (4 and 7, the lengths, are derived from 3 and 6).  A value is
        either a list of per-utterance numpy arrays (concatenated here with `align`-byte aligned starts) or an already flat field
        (flat, offsets, lens, row shape): `flat` a 1-D numpy array or device tensor, `offsets` in elements, `lens` in rows — taken
        as it is, in its own dtype."""
        self = cls.__new__(cls)
        built, n = {}, None
        for k in sorted(fields):
            v = fields[k]
            if isinstance(v, tuple):
                flat, offsets, lens, tail = v
                built[k] = (flat, np.asarray(offsets, dtype=np.int64), np.asarray(lens, dtype=np.int64), tuple(tail), k in SCALARS)
            else:
                built[k] = _flatten(k, v, ["utterance %d" % i for i in range(len(v))], align)
            n = len(built[k][2]) if n is None else n
            if len(built[k][2]) != n:
                raise ValueError("field %s has %d utterances, the others %d" % (NAMES.get(k, k), len(built[k][2]), n))
        ids = list(ids) if ids is not None else ["utt%d" % i for i in range(n)]
        self._build(built, ids, list(raw_texts) if raw_texts is not None else list(ids), device, max_gb)
        return self

    def _build(self, built, ids, raw_texts, device, max_gb):
        self.ids, self.raw_texts, self.device = ids, raw_texts, torch.device(device)
        n = len(ids)
        self.text_lens = np.asarray(built[3][2], dtype=np.int64)
        self.mel_lens = np.asarray(built[6][2], dtype=np.int64)
        for k, lens in ((4, self.text_lens), (7, self.mel_lens)):     # np.array of Python ints in `reprocess`: int64
            built[k] = (lens.copy(), np.arange(n, dtype=np.int64), np.ones(n, dtype=np.int64), (), True)
        if len(built) > 16:
            raise ValueError("%d fields: the collate kernel takes 16" % len(built))
        size = sum((f[0].numel() * f[0].element_size() if torch.is_tensor(f[0]) else f[0].nbytes) + 12 * n for f in built.values())
        if size > float(max_gb) * 2.0 ** 30:
            raise MemoryError("the resident training set needs %.3f GB on the device, more than mi355x.resident_max_gb = %g" % (
                size / 2.0 ** 30, float(max_gb)))
        self.fields = [_Field(k, *built[k], device=self.device) for k in sorted(built)]
        self.nbytes = sum(f.nbytes for f in self.fields)
        self._table = (L.CollateField * len(self.fields))()
        for row, f in zip(self._table, self.fields):
            row.src, row.offsets, row.lens, row.lens_host = f.flat.data_ptr(), f.offsets.data_ptr(), f.lens.data_ptr(), f.lens_host.ctypes.data
            row.n_src, row.elem_size, row.inner, row.nan_to_zero = f.flat.numel(), f.dtype.itemsize, f.inner, int(f.index in NAN_TO_ZERO)

    def __len__(self):
        return len(self.ids)

    def plan(self, indices, bucket=None):
        """Host side of a batch: (idx int32 array, {field index: target shape}, layout, total bytes, Lb, Tb, t_true, l_true) — what
        `reprocess` + `engine.bucket_plan` + `dataset.packed_layout` give for these utterances, from the lengths alone."""
        from .engine import bucket_plan
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        bad = idx[(idx < 0) | (idx >= len(self))]
        if idx.size == 0 or bad.size:
            raise IndexError("batch index %s outside the resident store's %d utterances" % (bad[:1].tolist() if bad.size else "[]", len(self)))
        B = idx.size
        max_src, max_mel = self.text_lens[idx].max(), self.mel_lens[idx].max()
        shapes = {f.index: (B,) + ((f.tail) if f.scalar else (int(f.lens_host[idx].max()),) + f.tail) for f in self.fields}
        Lb, Tb, t_true, l_true = max_src, max_mel, None, None
        if bucket is not None:
            # the numpy batch `bucket_plan` reads, as shapes without data: [5], [8] and axis 1 of energy / pitch
            shaped = [None] * 15
            shaped[5], shaped[8] = max_src, max_mel
            for k in (9, 11):
                shaped[k] = np.broadcast_to(np.zeros((), np.float32), shapes[k]) if k in shapes else np.zeros((B, 0), np.float32)
            Lb, Tb, t_true, l_true, axis1 = bucket_plan(shaped, *bucket)
            for k, n in axis1.items():
                if k in shapes:
                    shapes[k] = (B, n) + shapes[k][2:]
        arrays = [(f.index, np.empty(0, dtype=f.dtype), shapes[f.index]) for f in self.fields]
        if t_true is not None:
            arrays.append(("fl", np.empty(0, dtype=np.int32), (1,)))
        if l_true is not None:
            arrays.append(("pl", np.empty(0, dtype=np.int64), (B,)))
        layout, total = packed_layout(arrays)
        return idx.astype(np.int32), shapes, tuple(layout), total, Lb, Tb, t_true, l_true

    def batch(self, indices, bucket=None, idx_dev=None, out=None):
        """The PaddedBatch `DeviceFeeder(bucket=bucket)` yields for `reprocess([dataset[i] for i in indices], range(B))`: device fields
        as views of one `packed` buffer with `layout`, `frame_limit` / `phoneme_limit`, ids and raw texts as host lists.  One kernel
        launch on the current stream.  `idx_dev`: the same indices already on the device (int32; a slice of an uploaded plan) —
        without it they are uploaded here.  `out`: a uint8 device buffer of the batch's size to write into."""
        from .engine import PaddedBatch
        idx, shapes, layout, total, Lb, Tb, t_true, l_true = self.plan(indices, bucket)
        if idx_dev is None:
            idx_dev = torch.from_numpy(idx).to(self.device)
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=self.device)
        elif out.numel() != total:
            raise ValueError("batch buffer of %d bytes, the batch needs %d" % (out.numel(), total))
        offs = {tag: o for tag, o, _, _, _ in layout}
        for row, f in zip(self._table, self.fields):
            row.dst_off, row.padded_rows = offs[f.index], 1 if f.scalar else shapes[f.index][1]
        ops.collate_batch(self._table, len(self.fields), idx_dev, idx, len(self), out, offs.get("fl", -1), t_true or 0, offs.get("pl", -1), l_true or 0)
        views = views_of(out, layout)
        b = [None] * 15
        b[0], b[1] = [self.ids[i] for i in idx], [self.raw_texts[i] for i in idx]
        b[5], b[8] = Lb, Tb
        for f in self.fields:
            b[f.index] = views[f.index]
        b = PaddedBatch(b)
        b.t_true, b.l_true, b.frame_limit, b.phoneme_limit = t_true, l_true, views.get("fl"), views.get("pl")
        b.packed, b.layout = out, layout
        return b

    def batches(self, index_lists, bucket=None):
        """`batch` for every index list, their indices uploaded together, once, before the first."""
        index_lists = [np.asarray(ix, dtype=np.int32).reshape(-1) for ix in index_lists]
        if not index_lists:
            return
        plan = torch.from_numpy(np.concatenate(index_lists)).to(self.device)
        o = 0
        for ix in index_lists:
            yield self.batch(ix, bucket, idx_dev=plan[o:o + ix.size])
            o += ix.size


class ResidentLoader:
    """Iterates an epoch's PaddedBatches in the reference's order (`index_plan` of the sampler's indices; sampler None = the store's own
    order): per epoch one upload of the index plan, per batch one kernel launch on the current stream and no host-to-device copy."""

    def __init__(self, store, batch_size, group_size=4, sort=True, drop_last=True, sampler=None, bucket=None):
        self.store, self.batch_size, self.group_size, self.sort, self.drop_last = store, int(batch_size), int(group_size), sort, drop_last
        self.sampler, self.bucket = sampler, bucket

    def index_plan(self):
        order = list(self.sampler) if self.sampler is not None else range(len(self.store))
        return index_plan(order, self.store.text_lens, self.batch_size, self.group_size, self.sort, self.drop_last)

    def __iter__(self):
        return self.store.batches(self.index_plan(), self.bucket)
