"""Paragraphs: a text cut into sentences, the sentences synthesized as one batch and joined on the device.

Host planning only (numpy, no device): the splitter, the pauses, the groups, and the join table of ttsk_wav_join (include/ttsk.h).
A sentence is what the batched route is built for (`mel_ragged`, the windowed vocoder, short rows); the join turns the flat buffer
that route leaves on the device into one waveform: per sentence the silence at either end trimmed (threshold relative to the
sentence's peak), the level set (to a target RMS under a peak limit, to a peak, or by a given gain), a short linear fade at both
cuts, a pause behind it.  Everything that depends on a length or a setting is a number in the table, so one captured graph serves
every call with the same window count.

The join table is (1 + rows, ROW) 32-bit words, int32 with the fp32 fields stored by their bits:
    row 0      mode, fade, keep, lead, r, floor, target, limit                 (`Settings`)
    row 1 + u  src_off, src_len, pause, flags (bit 0: trim), gain, 0, 0, 0     (utterance u; src_len = 0: an empty padding row)
and the kernels answer with the info table, (rows + 1, ROW):
    row u      a, b, o_u, peak, ss, g, 0, 0        row `rows`: total, 0, ...
"""
import numpy as np

ROW = 8             # 32-bit words per row of the join table and of the info table (TTSK_JOIN_ROW)
MAX_ROWS = 4096     # TTSK_JOIN_MAX_ROWS
GIVEN, RMS, PEAK = 0, 1, 2          # TTSK_JOIN_GIVEN / _RMS / _PEAK
MODES = {None: GIVEN, "given": GIVEN, "rms": RMS, "peak": PEAK}
FLAG_TRIM = 1

ENDS = ".?!…"       # sentence ends
HALF = ";:"         # cuts inside a sentence
COMMA = ","         # cuts only a piece that is too long
PAUSES_MS = {"end": 400.0, "half": 250.0, "comma": 120.0}        # after ENDS (and after a piece nothing closes), HALF, COMMA
BATCH = 32          # sentences per call of the batched route (`mi355x.narrate_batch`)
MAX_PHONEMES = 200
TRIM_FLOOR_DB = -80.0       # the trim threshold never falls below this (relative to full scale): digital silence plus dither is silence


def default_count(piece):
    """Phonemes of a piece of text, as far as the host can tell without a frontend: the names inside {...}, one per other non-blank character."""
    n, pos = 0, 0
    while pos < len(piece):
        lb = piece.find("{", pos)
        rb = piece.find("}", lb + 1) if lb >= 0 else -1
        if lb < 0 or rb < 0:
            return n + sum(1 for c in piece[pos:] if not c.isspace())
        n += sum(1 for c in piece[pos:lb] if not c.isspace()) + len(piece[lb + 1:rb].split())
        pos = rb + 1
    return n


def _cut(text, marks):
    """(piece, mark) for every run of `text` that ends at one of `marks` outside {...} (a run of marks counts as its first: "?!",
    "..."), and the rest with mark ""."""
    out, depth, start, i = [], 0, 0, 0
    while i < len(text):
        c = text[i]
        if c == "{":
            depth += 1
        elif c == "}":
            depth = max(0, depth - 1)
        elif depth == 0 and c in marks:
            j = i + 1
            while j < len(text) and text[j] in ENDS + HALF + COMMA:
                j += 1
            out.append((text[start:i], c))
            start = i = j
            continue
        i += 1
    out.append((text[start:], ""))
    return out


def split_text(text, max_phonemes=MAX_PHONEMES, count=default_count):
    """A string -> (pieces, marks): cut at . ? ! … ; : outside {...}; a piece of more than `max_phonemes` phonemes (by `count`) also at
    its commas.  marks[i] is the punctuation that ended pieces[i] ("" for a piece that nothing closed).  A piece that is empty after
    stripping is dropped.  A list or tuple is taken as already split: its entries (strings or phoneme-id arrays) with mark "", empty
    ones dropped."""
    if isinstance(text, (list, tuple)):
        pieces = [t for t in text if (len(t.strip()) if isinstance(t, str) else np.asarray(t).size)]
        return pieces, [""] * len(pieces)
    if not isinstance(text, str):
        raise ValueError("split_text: text must be a string or a list of strings / phoneme-id arrays, got %s" % type(text).__name__)
    if int(max_phonemes) < 1:
        raise ValueError("split_text: max_phonemes must be at least 1, got %r" % (max_phonemes,))
    pieces, marks = [], []
    for piece, mark in _cut(text, ENDS + HALF):
        if not piece.strip():
            continue
        parts = [(piece, mark)]
        if count(piece) > max_phonemes:
            parts = _cut(piece, COMMA)
            parts[-1] = (parts[-1][0], mark)
        for p, m in parts:
            if p.strip():
                pieces.append(p.strip())
                marks.append(m)
    return pieces, marks


def ms_to_samples(ms, rate):
    """Milliseconds at `rate` Hz as a whole number of samples, halves rounded up."""
    return int(np.floor(float(ms) * int(rate) / 1000.0 + 0.5))


def pause_plan(marks, rate, pauses=None, configured=None):
    """Samples of pause behind every piece at the OUTPUT rate.  From each piece's mark (PAUSES_MS, overridden by `configured` =
    `mi355x.narrate_pauses`: a mapping with any of end / half / comma in ms), unless `pauses` is given: one number of ms for all, or
    one per piece."""
    n = len(marks)
    if pauses is None:
        table = dict(PAUSES_MS)
        for k, v in (configured or {}).items():
            if k not in table:
                raise ValueError("narrate_pauses: unknown key %r (end, half, comma)" % (k,))
            table[k] = float(v)
        ms = [table["half" if m and m in HALF else "comma" if m and m in COMMA else "end"] for m in marks]
    elif np.ndim(pauses) == 0:
        ms = [float(pauses)] * n
    else:
        ms = [float(p) for p in pauses]
        if len(ms) != n:
            raise ValueError("pauses: %d values for %d sentences" % (len(ms), n))
    if any(not np.isfinite(p) or p < 0 for p in ms):
        raise ValueError("pause must be a finite number of milliseconds >= 0, got %r" % (ms,))
    return [ms_to_samples(p, rate) for p in ms]


def groups(n, batch=BATCH):
    """[lo, hi) ranges of at most `batch` sentences covering n of them in order."""
    if int(batch) < 1:
        raise ValueError("narrate_batch must be at least 1, got %r" % (batch,))
    return [(lo, min(lo + int(batch), n)) for lo in range(0, n, int(batch))]


def _f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


class Settings:
    """Row 0 of the join table: mode (GIVEN / RMS / PEAK), fade, keep, lead (samples), r, floor, target, limit (fp32)."""

    def __init__(self, mode=GIVEN, fade=0, keep=0, lead=0, r=0.0, floor=0.0, target=1.0, limit=1.0, trim=True):
        for name, v in (("fade", fade), ("keep", keep), ("lead", lead)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 2 ** 31:
                raise ValueError("%s must be a whole number of samples in 0 .. 2^31 - 1, got %r" % (name, v))
        if mode not in (GIVEN, RMS, PEAK) or isinstance(mode, bool):
            raise ValueError("mode must be GIVEN, RMS or PEAK (0, 1, 2), got %r" % (mode,))
        for name, v in (("r", r), ("floor", floor)):
            if not np.isfinite(v) or v < 0:
                raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
        for name, v in (("target", target), ("limit", limit)):
            if not np.isfinite(v) or v <= 0:
                raise ValueError("%s must be finite and > 0, got %r" % (name, v))
        self.mode, self.fade, self.keep, self.lead = int(mode), int(fade), int(keep), int(lead)
        self.r, self.floor, self.target, self.limit = np.float32(r), np.float32(floor), np.float32(target), np.float32(limit)
        self.trim = bool(trim)

    def row(self):
        return [self.mode, self.fade, self.keep, self.lead] + [_f32_bits(v) for v in (self.r, self.floor, self.target, self.limit)]


def settings(rate, trim_db=-45.0, trim_keep_ms=15.0, fade_ms=5.0, normalize="rms", target_db=-23.0, peak_limit=0.95, lead_ms=0.0,
             trim_floor_db=TRIM_FLOOR_DB):
    """`narrate`'s arguments as `Settings` at `rate` Hz.  trim_db None: no trimming; normalize None: every gain 1 (mode GIVEN)."""
    if normalize not in MODES:
        raise ValueError("normalize must be \"rms\", \"peak\", \"given\" or None, got %r" % (normalize,))
    for name, v in (("trim_keep_ms", trim_keep_ms), ("fade_ms", fade_ms), ("lead_ms", lead_ms)):
        if not np.isfinite(v) or v < 0:
            raise ValueError("%s must be a finite number of milliseconds >= 0, got %r" % (name, v))
    if trim_db is not None and not (np.isfinite(trim_db) and trim_db <= 0):
        raise ValueError("trim_db must be a finite number of dB <= 0 (relative to the sentence's peak) or None, got %r" % (trim_db,))
    if not np.isfinite(target_db) or not (np.isfinite(peak_limit) and peak_limit > 0):
        raise ValueError("target_db must be finite and peak_limit finite and > 0, got %r, %r" % (target_db, peak_limit))
    trim = trim_db is not None
    return Settings(MODES[normalize], ms_to_samples(fade_ms, rate), ms_to_samples(trim_keep_ms, rate) if trim else 0, ms_to_samples(lead_ms, rate),
                    r=np.float32(10.0 ** (trim_db / 20.0)) if trim else 0.0, floor=np.float32(10.0 ** (trim_floor_db / 20.0)) if trim else 0.0,
                    target=np.float32(10.0 ** (target_db / 20.0)), limit=np.float32(peak_limit), trim=trim)


def join_table(src_offs, src_lens, pauses, st, rows=None, gains=None, trim=None):
    """The join table of utterances at `src_offs` (samples of the flat buffer) of `src_lens` samples with `pauses` samples behind
    them, under the settings `st`: (1 + rows, ROW) int32, padded with empty rows to `rows` (the capacity the caller names).  `gains`:
    one fp32 gain per utterance (mode GIVEN; default 1).  `trim`: one flag per utterance (default: `st.trim` for all)."""
    src_offs, src_lens, pauses = [int(o) for o in src_offs], [int(n) for n in src_lens], [int(p) for p in pauses]
    U = len(src_lens)
    if len(src_offs) != U or len(pauses) != U:
        raise ValueError("join_table: %d offsets, %d lengths and %d pauses must pair up" % (len(src_offs), U, len(pauses)))
    rows = U if rows is None else int(rows)
    if rows < U or not 1 <= rows <= MAX_ROWS:
        raise ValueError("join_table: %d utterances in %d rows: the rows must hold them and number 1 .. %d" % (U, rows, MAX_ROWS))
    for name, vals in (("src_off", src_offs), ("src_len", src_lens), ("pause", pauses)):
        if any(not 0 <= v < 2 ** 31 for v in vals):
            raise ValueError("join_table: every %s must be in 0 .. 2^31 - 1, got %r" % (name, [v for v in vals if not 0 <= v < 2 ** 31][:4]))
    if any(o + n >= 2 ** 31 for o, n in zip(src_offs, src_lens)):
        raise ValueError("join_table: the flat buffer must stay below 2^31 samples")
    gains = [1.0] * U if gains is None else [float(g) for g in gains]
    trim = [st.trim] * U if trim is None else [bool(t) for t in trim]
    if len(gains) != U or len(trim) != U or any(not np.isfinite(g) for g in gains):
        raise ValueError("join_table: one finite gain and one trim flag per utterance")
    t = np.zeros((1 + rows, ROW), dtype=np.int32)
    t[0] = st.row()
    for u in range(U):
        t[1 + u, :5] = (src_offs[u] if src_lens[u] else 0, src_lens[u], pauses[u], FLAG_TRIM if trim[u] else 0, _f32_bits(gains[u]))
    if out_bound(t) >= 2 ** 31:
        raise ValueError("join_table: the joined waveform may reach %d samples, the limit is 2^31 - 1" % out_bound(t))
    return t


class Join:
    """What a vocoder route needs to join the utterances of ONE call: the settings, and per utterance (in the call's order) the pause
    in samples at the output rate, optionally a gain (mode GIVEN) and a trim flag.  The route knows where its utterances lie and
    asks for the table (`table`)."""

    def __init__(self, st, pauses, gains=None, trim=None):
        self.st, self.pauses = st, [int(p) for p in pauses]
        self.gains = None if gains is None else [float(g) for g in gains]
        self.trim = None if trim is None else [bool(t) for t in trim]
        n = len(self.pauses)
        if not 1 <= n <= MAX_ROWS or any(v is not None and len(v) != n for v in (self.gains, self.trim)):
            raise ValueError("Join: 1 .. %d utterances, with one pause (and, where given, one gain and one trim flag) each" % MAX_ROWS)

    def __len__(self):
        return len(self.pauses)

    def part(self, lo, hi):
        """The join of the utterances [lo, hi) alone."""
        cut = lambda v: None if v is None else v[lo:hi]
        return Join(self.st, self.pauses[lo:hi], cut(self.gains), cut(self.trim))

    def table(self, src_offs, src_lens, rows=None):
        return join_table(src_offs, src_lens, self.pauses, self.st, rows, self.gains, self.trim)

    def pause_total(self):
        return self.st.lead + sum(self.pauses)


def out_bound(table):
    """Samples the joined waveform has at most: lead + every src_len + every pause (exact when nothing is trimmed)."""
    return int(table[0, 3]) + int(table[1:, 1].astype(np.int64).sum()) + int(table[1:, 2].astype(np.int64).sum())


class Info:
    """The info table on the host: per row a, b, o (int), peak, ss, g (fp32) as arrays over the `rows` given, and `total`."""

    def __init__(self, info, rows=None):
        info = np.asarray(info).reshape(-1, ROW)
        if info.dtype != np.int32:
            raise ValueError("Info: needs the int32 table as the kernels wrote it, got %s" % info.dtype)
        U = info.shape[0] - 1
        n = U if rows is None else int(rows)
        self.a, self.b, self.o = (info[:n, k].astype(np.int64) for k in range(3))
        self.peak, self.ss, self.g = (np.ascontiguousarray(info[:n, k]).view(np.float32) for k in (3, 4, 5))
        self.total = int(info[U, 0])

    def timing(self):
        """(start_sample, end_sample) of every row's kept samples in the joined waveform."""
        return [(int(o), int(o + b - a)) for a, b, o in zip(self.a, self.b, self.o)]
