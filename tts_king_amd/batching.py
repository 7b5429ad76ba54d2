"""Host-side shape logic of the batched text -> mel path (`GraphedSynthesizer.mel_ragged`, tts_king_amd/synth.py): which
utterances of a call run together, the phoneme / frame buckets they are padded to, the graph keys, and the per-utterance control
arrays.  numpy only -- importable and testable without a GPU.

The texts of a call are padded to a multiple of `mi355x.l_bucket` phonemes and the frame axis to a multiple of `mi355x.t_bucket`
frames (the training buckets: 8 and 32), both capped at `max_seq_len` (the length of the position tables; not a multiple of 32).
The graph keys hold the batch size and the buckets and nothing else: lengths, speakers and the three controls are VALUES the
graphs read from static device buffers.  An utterance whose text or predicted frame count exceeds `max_seq_len` cannot use the
position tables: it leaves the batch for the single-utterance path, which builds its own table.
"""
import numpy as np

L_BUCKET, T_BUCKET = 8, 32


def bucket(n, step, cap):
    """The smallest multiple of `step` that holds `n` (at least one step), capped at `cap`; `n` itself must not exceed `cap`."""
    n, step, cap = int(n), max(int(step), 1), int(cap)
    if n > cap:
        raise ValueError("%d exceeds the cap %d: such an utterance does not belong in the batch" % (n, cap))
    return min((max(n, 1) + step - 1) // step * step, cap)


def front_key(B, L_bucket):
    return ("front", int(B), int(L_bucket))


def back_key(B, L_bucket, T_bucket):
    return ("back", int(B), int(L_bucket), int(T_bucket))


def per_utterance(value, B, name, dtype=np.float32):
    """A control (or any per-utterance setting) as a (B,) array: a scalar is broadcast, a sequence must have B entries."""
    a = np.asarray(value, dtype=dtype)
    if a.ndim == 0:
        return np.full((B,), a, dtype=dtype)
    if a.ndim != 1 or a.shape[0] != B:
        raise ValueError("%s: expected a scalar or %d values (one per utterance), got shape %s" % (name, B, a.shape))
    return np.ascontiguousarray(a)


def per_utterance_names(value, B, name):
    """A speaker name (or None) for every utterance: one name is broadcast, a list must have B entries."""
    if value is None or isinstance(value, (str, int, np.integer)):
        return [value] * B
    value = list(value)
    if len(value) != B:
        raise ValueError("%s: expected one value or %d values (one per utterance), got %d" % (name, B, len(value)))
    return value


def as_id_rows(texts):
    """The texts of a call as a list of 1-D int64 arrays; a (1, L) array (what `text_preprocess` returns) counts as one text."""
    rows = []
    for t in texts:
        a = np.asarray(t)
        if a.ndim == 2 and a.shape[0] == 1:
            a = a[0]
        if a.ndim != 1 or a.shape[0] < 1:
            raise ValueError("every text must be a non-empty 1-D array of phoneme ids (or (1, L)), got shape %s" % (a.shape,))
        rows.append(np.ascontiguousarray(a, dtype=np.int64))
    if not rows:
        raise ValueError("an empty list of texts")
    return rows


class TextPlan:
    """`batch`: positions (in the call's order) of the utterances that run together, `solo`: of those over `max_seq_len`;
    `L`: the phoneme bucket; `ids` (len(batch), L) int64, zero-padded; `lens` (len(batch),) int64."""

    def __init__(self, batch, solo, L, ids, lens):
        self.batch, self.solo, self.L, self.ids, self.lens = batch, solo, L, ids, lens

    @property
    def key(self):
        return front_key(len(self.batch), self.L)


def plan_texts(texts, max_seq_len, l_bucket=L_BUCKET, only=None):
    """texts: a list of 1-D id arrays (`only`: the positions to consider, default all) -> TextPlan."""
    idx = list(range(len(texts))) if only is None else list(only)
    batch = [i for i in idx if len(texts[i]) <= max_seq_len]
    solo = [i for i in idx if len(texts[i]) > max_seq_len]
    if not batch:
        return TextPlan(batch, solo, 0, np.zeros((0, 0), np.int64), np.zeros((0,), np.int64))
    lens = np.array([len(texts[i]) for i in batch], dtype=np.int64)
    L = bucket(lens.max(), l_bucket, max_seq_len)
    ids = np.zeros((len(batch), L), dtype=np.int64)
    for r, i in enumerate(batch):
        ids[r, :lens[r]] = texts[i]
    return TextPlan(batch, solo, L, ids, lens)


def plan_frames(totals, max_seq_len, t_bucket=T_BUCKET):
    """totals: the predicted frame counts of the batch's utterances (host) -> (rows that stay, rows over `max_seq_len`, the frame
    bucket of those that stay or 0 when none does)."""
    totals = [int(t) for t in totals]
    keep = [r for r, t in enumerate(totals) if t <= max_seq_len]
    over = [r for r, t in enumerate(totals) if t > max_seq_len]
    T = bucket(max(totals[r] for r in keep), t_bucket, max_seq_len) if keep else 0
    return keep, over, T
