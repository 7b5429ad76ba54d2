"""A minimal reader for Praat TextGrids in the *long* text format (what the Montreal Forced Aligner writes), and the reference's
alignment rules on top of it (fs_two/preprocessor/preprocessor.py:313-349, which reads the file with the `tgt` package).

The long format names every field:

    File type = "ooTextFile"
    Object class = "TextGrid"
    ...
    item [1]:
        class = "IntervalTier"
        name = "phones"
        intervals: size = 3
        intervals [1]:
            xmin = 0
            xmax = 0.25
            text = "sil"

The short format (bare values, one per line), binary TextGrids and point tiers are refused by name."""
import re

import numpy as np

SIL_PHONES = ("sil", "sp", "spn")


class TextGridError(ValueError):
    pass


_ITEM = re.compile(r"^\s*item\s*\[(\d+)\]\s*:", re.M)
_INTERVAL = re.compile(r"intervals\s*\[(\d+)\]\s*:\s*xmin\s*=\s*([-+0-9.eE]+)\s*xmax\s*=\s*([-+0-9.eE]+)\s*text\s*=\s*\"((?:[^\"]|\"\")*)\"")


def _decode(raw, path):
    if raw[:2] in (b"\xff\xfe", b"\xfe\xff"):
        return raw.decode("utf-16")
    if raw[:3] == b"\xef\xbb\xbf":
        return raw[3:].decode("utf-8")
    if raw.startswith(b"ooBinaryFile"):
        raise TextGridError("%s: a binary TextGrid; only Praat's long text format is read" % path)
    return raw.decode("utf-8")


def parse(text, path="<string>"):
    """{tier name: [(xmin, xmax, text), ...]} of every interval tier of a long-format TextGrid."""
    head = text[:400]
    if "ooTextFile" not in head or '"TextGrid"' not in head:
        raise TextGridError("%s: not a Praat TextGrid (no ooTextFile / TextGrid header)" % path)
    if not re.search(r"^\s*xmin\s*=", text, re.M) or not _ITEM.search(text):
        raise TextGridError("%s: a short-format TextGrid (bare values without `xmin =` / `item [n]:`); only Praat's long text format is "
                            "read -- save it from Praat as a text file, not a short text file" % path)
    tiers = {}
    marks = list(_ITEM.finditer(text))
    for i, m in enumerate(marks):
        body = text[m.end():marks[i + 1].start() if i + 1 < len(marks) else len(text)]
        cls = re.search(r"class\s*=\s*\"([^\"]*)\"", body)
        name = re.search(r"name\s*=\s*\"((?:[^\"]|\"\")*)\"", body)
        if cls is None or name is None:
            raise TextGridError("%s: item [%s] has no class or name" % (path, m.group(1)))
        if cls.group(1) != "IntervalTier":
            continue                               # point tiers carry no durations
        size = re.search(r"intervals\s*:\s*size\s*=\s*(\d+)", body)
        ivs = [(float(a), float(b), t.replace('""', '"')) for _, a, b, t in _INTERVAL.findall(body)]
        if size is None or int(size.group(1)) != len(ivs):
            raise TextGridError("%s: tier %r announces %s intervals, %d were read" % (path, name.group(1), size.group(1) if size else "no", len(ivs)))
        tiers[name.group(1).replace('""', '"')] = ivs
    return tiers


def read_tier(path, tier="phones"):
    """The intervals [(xmin, xmax, text), ...] of the interval tier `tier` of the long-format TextGrid at `path`."""
    with open(path, "rb") as f:
        tiers = parse(_decode(f.read(), path), path)
    if tier not in tiers:
        raise TextGridError("%s: no interval tier named %r (it has %s)" % (path, tier, sorted(tiers)))
    return tiers[tier]


def get_alignment(intervals, sampling_rate, hop_length):
    """(phones, durations, start_time, end_time) by the reference's rules: leading sil / sp / spn are dropped, trailing ones too, an
    inner one stays; a phone's frames are round(e sr / hop) - round(s sr / hop) (numpy's round: halves to even)."""
    phones, durations = [], []
    start_time = end_time = 0
    end_idx = 0
    for s, e, p in intervals:
        if not phones:
            if p in SIL_PHONES:
                continue
            start_time = s
        phones.append(p)
        if p not in SIL_PHONES:
            end_time = e
            end_idx = len(phones)
        durations.append(int(np.round(e * sampling_rate / hop_length) - np.round(s * sampling_rate / hop_length)))
    return phones[:end_idx], durations[:end_idx], start_time, end_time
