"""CPU: the host planning of paragraphs (tts_king_amd/narrate.py) and the numpy restatement of the join (tests/join_ref.py) on cases
worked out by hand.  No device."""
import re

import numpy as np
import pytest

from tests import join_ref as ref
from tts_king_amd import lib, narrate

F32 = np.float32


def test_constants_match_the_header():
    with open(lib.HEADER_PATH) as f:
        text = f.read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert narrate.ROW == val("TTSK_JOIN_ROW") and narrate.MAX_ROWS == val("TTSK_JOIN_MAX_ROWS")
    assert (narrate.GIVEN, narrate.RMS, narrate.PEAK) == (val("TTSK_JOIN_GIVEN"), val("TTSK_JOIN_RMS"), val("TTSK_JOIN_PEAK"))


# ------------------------------------------------------------------------------------------------ the splitter

def test_split_at_sentence_marks_and_returns_them():
    pieces, marks = narrate.split_text("{A B}. {V G}? {D}! {E}… {Z}; {I}: {K}")
    assert pieces == ["{A B}", "{V G}", "{D}", "{E}", "{Z}", "{I}", "{K}"]
    assert marks == [".", "?", "!", "…", ";", ":", ""]


def test_braces_are_never_cut():
    pieces, marks = narrate.split_text("{A . B , V ; G}. {D ! E}")
    assert pieces == ["{A . B , V ; G}", "{D ! E}"] and marks == [".", ""]


def test_comma_only_cuts_a_piece_that_is_too_long():
    text = "{A B V}, {G D}. {E}, {Z}."
    assert narrate.split_text(text) == (["{A B V}, {G D}", "{E}, {Z}"], [".", "."])
    # 5 phonemes and a comma count 6 > 4; the second sentence counts 3 and stays whole
    pieces, marks = narrate.split_text(text, max_phonemes=4)
    assert pieces == ["{A B V}", "{G D}", "{E}, {Z}"] and marks == [",", ".", "."]
    # the caller's count decides
    pieces, marks = narrate.split_text(text, max_phonemes=1, count=lambda p: 2)
    assert pieces == ["{A B V}", "{G D}", "{E}", "{Z}"] and marks == [",", ".", ",", "."]


def test_empty_pieces_are_dropped_and_mark_runs_count_once():
    pieces, marks = narrate.split_text("  . {A}?!  ... {B} ;; ")
    assert pieces == ["{A}", "{B}"] and marks == ["?", ";"]
    assert narrate.split_text("") == ([], []) and narrate.split_text(" .;, ") == ([], [])


def test_a_list_is_taken_as_split():
    ids = np.array([[3, 4, 5]])
    pieces, marks = narrate.split_text(["{A}. {B}", "  ", ids, np.zeros((1, 0), np.int64)])
    assert len(pieces) == 2 and pieces[0] == "{A}. {B}" and pieces[1] is ids and marks == ["", ""]
    with pytest.raises(ValueError, match="split_text: text must be"):
        narrate.split_text(7)
    with pytest.raises(ValueError, match="max_phonemes"):
        narrate.split_text("{A}", max_phonemes=0)


def test_default_count():
    assert narrate.default_count("{A B V} x y, {G}") == 3 + 3 + 1


# ------------------------------------------------------------------------------------------------ pauses, groups

def test_pause_plan_at_two_rates():
    marks = [".", "?", "!", "…", ";", ":", ",", ""]
    assert narrate.pause_plan(marks, 22050) == [8820] * 4 + [5512 + 1] * 2 + [2646, 8820]       # 250 ms = 5512.5 samples: halves up
    assert narrate.pause_plan(marks, 16000) == [6400] * 4 + [4000] * 2 + [1920, 6400]
    assert narrate.pause_plan(marks, 16000, configured={"half": 100, "comma": 0}) == [6400] * 4 + [1600] * 2 + [0, 6400]
    assert narrate.pause_plan([".", ","], 22050, pauses=100) == [2205, 2205]
    assert narrate.pause_plan([".", ",", ""], 16000, pauses=[100, 0, 50.5]) == [1600, 0, 808]
    assert narrate.pause_plan([".", ",", ""], 16000, pauses=[100, 0, 50], configured={"end": 1}) == [1600, 0, 800]


def test_pause_refusals_by_name():
    with pytest.raises(ValueError, match="pauses: 2 values for 3 sentences"):
        narrate.pause_plan([".", ".", "."], 22050, pauses=[1, 2])
    with pytest.raises(ValueError, match="pause must be .* >= 0"):
        narrate.pause_plan(["."], 22050, pauses=-1)
    with pytest.raises(ValueError, match="pause must be"):
        narrate.pause_plan(["."], 22050, pauses=[float("nan")])
    with pytest.raises(ValueError, match="narrate_pauses: unknown key 'stop'"):
        narrate.pause_plan(["."], 22050, configured={"stop": 3})


def test_groups_of_32():
    assert narrate.groups(1) == [(0, 1)] and narrate.groups(32) == [(0, 32)]
    assert narrate.groups(33) == [(0, 32), (32, 33)] and narrate.groups(65) == [(0, 32), (32, 64), (64, 65)]
    assert narrate.groups(5, 2) == [(0, 2), (2, 4), (4, 5)] and narrate.groups(0) == []
    with pytest.raises(ValueError, match="narrate_batch"):
        narrate.groups(3, 0)


# ------------------------------------------------------------------------------------------------ settings and the table

def test_settings_from_narrate_arguments():
    st = narrate.settings(22050)
    assert (st.mode, st.fade, st.keep, st.lead, st.trim) == (narrate.RMS, 110, 331, 0, True)      # 5 ms = 110.25, 15 ms = 330.75
    assert st.r == F32(10.0 ** (-45.0 / 20.0)) and st.floor == F32(1e-4) and st.target == F32(10.0 ** (-23.0 / 20.0)) and st.limit == F32(0.95)
    st = narrate.settings(16000, trim_db=None, normalize=None, fade_ms=0)
    assert (st.mode, st.fade, st.keep, st.trim) == (narrate.GIVEN, 0, 0, False)
    assert narrate.settings(16000, normalize="peak").mode == narrate.PEAK
    for kw, name in ((dict(fade_ms=-1), "fade_ms"), (dict(trim_keep_ms=-0.5), "trim_keep_ms"), (dict(normalize="lufs"), "normalize"),
                     (dict(trim_db=3.0), "trim_db"), (dict(peak_limit=0.0), "peak_limit"), (dict(target_db=float("inf")), "target_db")):
        with pytest.raises(ValueError, match=name):
            narrate.settings(22050, **kw)


def test_settings_refusals_by_name():
    for kw, name in ((dict(fade=-1), "fade"), (dict(keep=-2), "keep"), (dict(lead=2 ** 31), "lead"), (dict(fade=1.5), "fade"), (dict(mode=3), "mode"),
                     (dict(r=-0.1), "r must"), (dict(floor=float("nan")), "floor"), (dict(target=0.0), "target"), (dict(limit=-1.0), "limit")):
        with pytest.raises(ValueError, match=name):
            narrate.Settings(**kw)


def test_table_layout_and_padding():
    st = narrate.Settings(narrate.RMS, fade=7, keep=3, lead=2, r=0.25, floor=0.5, target=0.125, limit=0.75)
    t = narrate.join_table([5, 100, 0], [10, 0, 20], [1, 2, 3], st, rows=6, gains=[1.0, 2.0, 0.5], trim=[True, False, True])
    assert t.dtype == np.int32 and t.shape == (7, narrate.ROW)
    assert t[0, :4].tolist() == [narrate.RMS, 7, 3, 2] and t[0, 4:].view(F32).tolist() == [0.25, 0.5, 0.125, 0.75]
    assert t[1].tolist() == [5, 10, 1, 1, F32(1.0).view(np.int32), 0, 0, 0]
    assert t[2].tolist() == [0, 0, 2, 0, F32(2.0).view(np.int32), 0, 0, 0]            # an empty row keeps its pause, its offset is dropped
    assert t[3].tolist() == [0, 20, 3, 1, F32(0.5).view(np.int32), 0, 0, 0]
    assert not t[4:].any()                                                          # padding rows: all zero
    assert narrate.out_bound(t) == 2 + 30 + 6
    assert narrate.join_table([0], [4], [0], st).shape == (2, narrate.ROW)           # rows default to the utterances


def test_table_refusals_by_name():
    st = narrate.Settings()
    for args, kw, name in ((([0], [1], [-1]), {}, "pause"), (([-1], [1], [0]), {}, "src_off"), (([0], [-1], [0]), {}, "src_len"),
                           (([0, 1], [1], [0]), {}, "pair up"), (([0, 1], [1, 1], [0, 0]), dict(rows=1), "rows"),
                           (([0], [1], [0]), dict(rows=4097), "1 .. 4096"), (([0], [1], [0]), dict(gains=[float("inf")]), "gain"),
                           (([2 ** 31 - 2], [5], [0]), {}, "below 2\\^31"), (([0, 0], [2 ** 30, 2 ** 30], [0, 0]), {}, "2\\^31 - 1")):
        with pytest.raises(ValueError, match=name):
            narrate.join_table(*args, st, **kw)
    with pytest.raises(ValueError, match="Join"):
        narrate.Join(st, [])
    with pytest.raises(ValueError, match="Join"):
        narrate.Join(st, [1, 2], gains=[1.0])


def test_join_parts():
    st = narrate.Settings(lead=4)
    j = narrate.Join(st, [1, 2, 3], gains=[1.0, 2.0, 3.0])
    p = j.part(1, 3)
    assert len(p) == 2 and p.pauses == [2, 3] and p.gains == [2.0, 3.0] and p.st is st and j.pause_total() == 10
    assert p.table([0, 8], [8, 8]).shape == (3, narrate.ROW)


def test_info_decodes_the_device_table():
    raw = np.zeros((3, narrate.ROW), np.int32)
    raw[0, :3] = (2, 9, 4)
    raw[0, 3:6] = np.array([0.5, 1.25, 2.0], F32).view(np.int32)
    raw[1, :3] = (0, 0, 11)
    raw[2, 0] = 30
    info = narrate.Info(raw)
    assert info.timing() == [(4, 11), (11, 11)] and info.total == 30
    assert info.peak.tolist() == [0.5, 0.0] and info.ss.tolist() == [1.25, 0.0] and info.g.tolist() == [2.0, 0.0]
    assert narrate.Info(raw, rows=1).timing() == [(4, 11)]


# ------------------------------------------------------------------------------------------------ the restatement, by hand

def _st(**kw):
    base = dict(mode=narrate.GIVEN, fade=0, keep=0, lead=0, r=0.5, floor=0.0, target=0.25, limit=1.0)
    base.update(kw)
    return narrate.Settings(**base)


def test_restatement_trim_and_layout_by_hand():
    x = np.array([9, 0.0, 0.1, 1.0, -0.5, 0.2, 0.0, 9, 9, 0.0, 0.0, 9, 0.25, 9], F32)
    #               ^ utterance 0 at 1, 6 samples     ^ utterance 1 at 9, 2 zeros   ^ utterance 2 at 12, 1 sample
    table = narrate.join_table([1, 9, 12], [6, 2, 1], [2, 1, 3], _st(keep=1, lead=1), rows=4, gains=[2.0, 1.0, 4.0])
    got = ref.join_ref(x, table, 16)
    # utterance 0: peak 1, thr 0.5, first = 2 (1.0), last = 3 (-0.5) -> a = 1, b = 5; utterance 1: peak 0 -> empty; utterance 2: kept
    assert got["a"].tolist() == [1, 0, 0, 0] and got["b"].tolist() == [5, 0, 1, 0]
    assert got["o"].tolist() == [1, 7, 8, 12] and got["total"] == 12 and got["timing"] == [(1, 5), (7, 7), (8, 9), (12, 12)]
    assert got["peak"].tolist() == [1.0, 0.0, 0.25, 0.0] and got["g"].tolist() == [2.0, 1.0, 4.0, 1.0]
    assert got["out"].tolist() == np.array([0, 0.2, 2.0, -1.0, 0.4, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 0], F32).tolist()    # doubling is exact
    assert got["ss64"][0] == pytest.approx(0.01 + 1 + 0.25 + 0.04, rel=1e-6)
    # without the trim flag everything is kept
    table = narrate.join_table([1, 9, 12], [6, 2, 1], [0, 0, 0], _st(trim=False), gains=[1.0, 1.0, 1.0])
    got = ref.join_ref(x, table, 9)
    assert got["a"].tolist() == [0, 0, 0] and got["b"].tolist() == [6, 2, 1] and got["total"] == 9
    assert got["out"].tolist() == x[[1, 2, 3, 4, 5, 6, 9, 10, 12]].tolist()


def test_restatement_floor_keeps_a_quiet_row_out():
    x = np.array([0.001, 0.002, 0.001], F32)
    got = ref.join_ref(x, narrate.join_table([0], [3], [2], _st(floor=0.01)), 4)
    assert got["b"].tolist() == [0] and got["total"] == 2 and not got["out"].any() and got["g"].tolist() == [1.0]


def test_restatement_fade_by_hand():
    x = np.ones(8, F32)
    got = ref.join_ref(x, narrate.join_table([0], [8], [0], _st(fade=2, trim=False)), 8)
    assert got["out"].tolist() == [0.25, 0.75, 1, 1, 1, 1, 0.75, 0.25]
    # a fade longer than half the kept range: F = 5 // 2 = 2, the middle sample stays whole
    got = ref.join_ref(x, narrate.join_table([0], [5], [0], _st(fade=100, trim=False)), 5)
    assert got["out"].tolist() == [0.25, 0.75, 1, 0.75, 0.25]
    # one sample: F = 0
    assert ref.join_ref(x, narrate.join_table([3], [1], [0], _st(fade=7, trim=False)), 1)["out"].tolist() == [1.0]
    assert ref.fade_weights(6, 3).tolist() == [F32(1) / F32(6), 0.5, F32(5) / F32(6), F32(5) / F32(6), 0.5, F32(1) / F32(6)]


def test_restatement_gains_by_hand():
    x = np.array([0.5, -0.5, 0.5, -0.5, 0.0, 0.0, 0.0, 1.0], F32)
    table = narrate.join_table([0, 4], [4, 4], [0, 0], _st(mode=narrate.RMS, trim=False, target=0.25, limit=1.0))
    got = ref.join_ref(x, table, 8)
    # row 0: rms 0.5 -> 0.25 / 0.5 = 0.5 (the limit allows 2); row 1: rms 0.5 too, but the peak 1 under limit 1 allows only 1 ... and 0.5 < 1
    assert got["g"].tolist() == [0.5, 0.5] and got["out"].tolist() == [0.25, -0.25, 0.25, -0.25, 0, 0, 0, 0.5]
    got = ref.join_ref(x, narrate.join_table([0, 4], [4, 4], [0, 0], _st(mode=narrate.RMS, trim=False, target=0.25, limit=0.25)), 8)
    assert got["g"].tolist() == [0.5, 0.25]                                        # row 1: the peak limit binds
    got = ref.join_ref(x, narrate.join_table([0, 4], [4, 4], [0, 0], _st(mode=narrate.PEAK, trim=False, limit=0.75)), 8)
    assert got["g"].tolist() == [1.5, 0.75] and got["out"][7] == 0.75
    # an all-zero row that is not trimmed: peak 0 -> gain 1, zeros out (never 0 * inf)
    got = ref.join_ref(np.zeros(4, F32), narrate.join_table([0], [4], [0], _st(mode=narrate.RMS, trim=False)), 4)
    assert got["g"].tolist() == [1.0] and not got["out"].any()


def test_restatement_int16_saturates_then_truncates():
    x = np.array([0.99999, -0.99999, 0.5, 2.0, -2.0, 1e-5], F32)
    got = ref.join_ref(x, narrate.join_table([0], [6], [1], _st(trim=False)), 8, int16_scale=32768.0)
    assert got["out"].dtype == np.int16 and got["out"].tolist() == [32767, -32767, 16384, 32767, -32768, 0, 0, 0]


def test_restatement_skips_a_row_outside_the_buffer_and_cuts_at_the_destination():
    x = np.arange(1, 9, dtype=F32)
    table = narrate.join_table([0, 6], [4, 4], [1, 1], _st(trim=False))
    got = ref.join_ref(x, table, 3)
    assert got["b"].tolist() == [4, 0] and got["total"] == 6 and got["out"].tolist() == [1, 2, 3]


def test_bounds_grow_with_the_reduction():
    assert ref.ss_bound(1) == ref.ss_bound(4096) < ref.ss_bound(4097) and ref.ss_bound(4096) == pytest.approx(25 * 2.0 ** -24, rel=1e-5)
    assert ref.gain_bound(20000) > ref.ss_bound(20000) / 2
