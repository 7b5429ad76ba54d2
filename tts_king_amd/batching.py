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


# ---------------------------------------------------------------------------------------------- per-phoneme prosody
# `mel_ragged(..., durations=, pitch=, energy=, target_frames=)` and per-phoneme arrays in the three controls.
# Every argument is None, a scalar, or one entry per utterance; an entry is None, a scalar or an array over the utterance's own
# phonemes in which NaN means "not set here".  The graphs of that route read all of it from (B, L_bucket) device arrays.

CONTROLS = ("p_control", "e_control", "d_control")
VALUES = ("pitch", "energy", "durations")


def rows_key(B, L_bucket):
    """The front graph of the per-phoneme route: one per shape, whatever inputs are given and whatever their values."""
    return ("front", int(B), int(L_bucket), "rows")


def _is_scalar(x):
    if isinstance(x, (bool, int, float, np.number)):
        return True
    return hasattr(x, "ndim") and not isinstance(x, (list, tuple)) and x.ndim == 0


def wants_rows(B, controls, values, target_frames):
    """Does a call need the per-phoneme route?  Yes when an explicit value or a frame budget is given, or when a control is
    anything but a scalar or B scalars (today's forms, which keep today's route)."""
    if target_frames is not None or any(v is not None for v in values):
        return True
    for c in controls:
        if c is None or _is_scalar(c):
            continue
        if isinstance(c, np.ndarray) and c.ndim == 1 and c.dtype != object:
            continue
        if isinstance(c, (list, tuple)) and all(_is_scalar(x) for x in c):
            continue
        return True
    return False


def _entries(value, B, name):
    """One entry per utterance out of None / a scalar / a sequence of B entries."""
    if value is None or _is_scalar(value):
        return [value] * B
    if isinstance(value, np.ndarray) and value.dtype != object:
        value = list(value)
    try:
        value = list(value)
    except TypeError:
        raise ValueError("%s: expected None, a scalar or %d entries (one per utterance), got %r" % (name, B, type(value).__name__))
    if len(value) != B:
        raise ValueError("%s: expected a scalar or %d entries (one per utterance), got %d" % (name, B, len(value)))
    return value


def _phoneme_row(entry, n, name, u, fill):
    """One utterance's entry as (values (n,) fp32, set (n,) bool): None -> nothing set, a scalar -> every phoneme, an array of n with
    NaN = not set.  Unset positions hold `fill`.  Infinite values are refused."""
    what = "%s[%d]" % (name, u)
    if entry is None:
        return np.full((n,), fill, np.float32), np.zeros((n,), bool)
    try:
        a = np.asarray(entry.detach().cpu().numpy() if hasattr(entry, "detach") else entry, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("%s: expected a scalar or %d numbers (one per phoneme)" % (what, n))
    if a.ndim == 0:
        a = np.full((n,), a, np.float32)
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError("%s: expected a scalar or %d values (one per phoneme of utterance %d), got shape %s" % (what, n, u, a.shape))
    if np.isinf(a).any():
        raise ValueError("%s: values must be finite (NaN marks a phoneme as not set), got an infinite value at phoneme %d"
                         % (what, int(np.flatnonzero(np.isinf(a))[0])))
    has = ~np.isnan(a)
    return np.where(has, a, np.float32(fill)).astype(np.float32), has


class Prosody:
    """The normalised per-phoneme inputs of a call, per utterance (texts over the phoneme bucket included): `ctl[k][u]` (len_u,) fp32
    for k = pitch, energy, duration control; `val[k][u]` / `has[k][u]` the explicit pitch, energy and durations and where they are
    set; `target` (B,) int32, -1 = no frame budget."""

    def __init__(self, lens, ctl, val, has, target):
        self.lens, self.ctl, self.val, self.has, self.target = lens, ctl, val, has, target

    def plain(self, u):
        """(p, e, d) scalar controls when utterance u carries nothing the scalar route cannot express, else None."""
        if self.target[u] >= 0 or any(self.has[k][u].any() for k in range(3)):
            return None
        if any(self.lens[u] > 0 and (self.ctl[k][u] != self.ctl[k][u][0]).any() for k in range(3)):
            return None
        return tuple(float(self.ctl[k][u][0]) for k in range(3))

    def padded(self, sel, L):
        """The ten (len(sel), L) / (len(sel),) arrays `FastSpeech2.eval_front_rows` takes, in its order.  Padding is neutral: control
        1, nothing set (value 0), target -1."""
        n = len(sel)
        out = []
        for k in range(3):
            c, v, h = np.ones((n, L), np.float32), np.zeros((n, L), np.float32), np.zeros((n, L), np.uint8)
            for r, u in enumerate(sel):
                m = self.lens[u]
                c[r, :m], v[r, :m], h[r, :m] = self.ctl[k][u], self.val[k][u], self.has[k][u]
            out += [c, v, h]
        out.append(np.ascontiguousarray(self.target[list(sel)], dtype=np.int32))
        return out


def plan_prosody(lens, p_control=1.0, e_control=1.0, d_control=1.0, pitch=None, energy=None, durations=None, target_frames=None):
    """Validate and normalise the prosody arguments of a call whose utterances have `lens` phonemes -> Prosody.  Raises ValueError
    naming the argument and the utterance: a wrong number of entries or phonemes, an infinite value, a negative duration, a frame
    budget that is no integer >= 0."""
    lens = [int(n) for n in lens]
    B = len(lens)
    ctl, val, has = [], [], []
    for name, arg in zip(CONTROLS, (p_control, e_control, d_control)):
        ent = _entries(1.0 if arg is None else arg, B, name)
        ctl.append([_phoneme_row(ent[u], lens[u], name, u, 1.0)[0] for u in range(B)])
    for name, arg in zip(VALUES, (pitch, energy, durations)):
        ent = _entries(arg, B, name)
        rows = [_phoneme_row(ent[u], lens[u], name, u, 0.0) for u in range(B)]
        if name == "durations":
            for u, (a, h) in enumerate(rows):
                if (a[h] < 0).any():
                    raise ValueError("durations[%d]: frame counts must be >= 0, got %g at phoneme %d" % (u, a[h].min(), int(np.flatnonzero(h & (a < 0))[0])))
        val.append([r[0] for r in rows])
        has.append([r[1].astype(np.uint8) for r in rows])
    target = np.full((B,), -1, np.int32)
    for u, t in enumerate(_entries(target_frames, B, "target_frames")):
        if t is None:
            continue
        f = float(t) if _is_scalar(t) else float("nan")
        if not (f >= 0 and f == int(f) and f < 2 ** 31):
            raise ValueError("target_frames[%d]: expected None or an integer >= 0, got %r" % (u, t))
        target[u] = int(f)
    return Prosody(lens, ctl, val, has, target)
