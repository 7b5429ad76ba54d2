"""CPU: the ground per-phoneme prosody stands on (`GraphedSynthesizer.mel_ragged` with per-phoneme controls,
explicit values and a frame budget).

1. The three entry points are declared in include/ttsk.h, exported, and refuse null pointers and bad sizes on the host.
2. The host-side normalisation (tts_king_amd/batching.py `plan_prosody`): forms, NaN = not set, neutral padding, every refusal, and a
   front key that depends on the shape alone.
3. The semantics the GPU test compares against, on the oracle: (1, L) control tensors broadcast per phoneme.
4. The fit rule, stated in numpy (`fit_rule`, which tests/test_prosody_gpu.py imports), against hand-worked cases.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fs2 as ofs2
from tests.test_batch_synth_cpu import oracle_weights
from tts_king_amd import batching, lib

NEW_SYMBOLS = ("ttsk_embed_step_rows", "ttsk_duration_rows", "ttsk_duration_fit")


def fit_rule(v, has, target):
    """The frame-budget rule of the issue for ONE utterance (its own phonemes only), fp64: v (n,) fp32 durations, has (n,) bool = the
    explicitly set (fixed) phonemes, target an int (< 0: none).  -> (n,) float64."""
    v = np.asarray(v, np.float32).astype(np.float64)
    fixed = np.asarray(has, bool)
    if target < 0:
        return v.copy()
    out = np.zeros_like(v)
    out[fixed] = np.trunc(v[fixed])
    F = out[fixed].sum()
    free = np.flatnonzero(~fixed & (v > 0))             # a free phoneme with v = 0 stays 0
    S = v[free].sum()
    budget = max(float(target) - F, 0.0)
    if S == 0 or len(free) == 0:
        return out
    q = v[free] * budget / S
    fl = np.floor(q)
    r = int(round(budget - fl.sum()))
    assert 0 <= r < max(len(free), 1) or r == 0
    order = np.argsort(-(q - fl), kind="stable")        # largest fractional part first, ties to the lower l
    fl[order[:r]] += 1
    out[free] = fl
    return out


def test_new_entry_points_are_declared_and_exported():
    protos = lib.declared_prototypes()
    l = lib.load()
    for name in NEW_SYMBOLS:
        assert name in protos and protos[name], name
        assert hasattr(l, name), name
        zero = [(None if a is lib.C.c_void_p else (0.0 if a in (lib.C.c_float, lib.C.c_double) else 0)) for a in protos[name]]
        assert getattr(l, name)(*zero) != 0, name + " accepted an all-null / all-zero argument list"


def test_null_pointers_and_bad_sizes_are_refused_on_the_host():
    """Every call here fails an argument check, which returns before any launch: nothing touches a device."""
    l = lib.load()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)           # a valid host address; never dereferenced
    good = {
        "ttsk_embed_step_rows": [p, p, p, p, p, 255, p, p, p, 8, p, p, p, 24, 256, None],
        "ttsk_duration_rows": [p, p, p, p, p, 24, None],
        "ttsk_duration_fit": [p, p, p, p, 8, p, 3, None],
    }
    protos = lib.declared_prototypes()
    for name, args in good.items():
        fn = getattr(l, name)
        assert len(args) == len(protos[name]), name
        for i, a in enumerate(args[:-1]):                      # each pointer in turn null (the stream may be null)
            if protos[name][i] is C.c_void_p:
                bad = list(args)
                bad[i] = None
                assert fn(*bad) != 0, "%s accepted a null argument %d" % (name, i)
                assert b"null" in l.ttsk_last_error()
    sizes = {
        "ttsk_embed_step_rows": [(5, 0), (9, 0), (9, 7), (13, 0), (13, 25), (14, 0), (14, 254)],   # n_bins, seg_len, rows % seg_len, rows, D, D % 4
        "ttsk_duration_rows": [(5, 0), (5, -3)],
        "ttsk_duration_fit": [(4, 0), (4, 1025), (6, 0), (6, -1)],
    }
    for name, cases in sizes.items():
        for i, v in cases:
            bad = list(good[name])
            bad[i] = v
            assert getattr(l, name)(*bad) != 0, "%s accepted argument %d = %d" % (name, i, v)


# ------------------------------------------------------------------------------------------------ host normalisation
LENS = (5, 3, 8)


def test_forms_padding_and_nan():
    nan = float("nan")
    p = batching.plan_prosody(LENS, p_control=1.5, e_control=[0.9, 1.0, 1.1], d_control=[np.linspace(1, 2, 5), None, 0.5],
                              pitch=[None, [1.0, nan, 3.0], None], energy=None, durations=[[nan, 4, nan, 0, nan], None, 2.0],
                              target_frames=[None, 7, 0])
    pc, pv, ph, ec, ev, eh, dc, dv, dh, tgt = p.padded([0, 1, 2], 8)
    for a in (pc, pv, ec, ev, dc, dv):
        assert a.shape == (3, 8) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    for a in (ph, eh, dh):
        assert a.shape == (3, 8) and a.dtype == np.uint8
    assert tgt.dtype == np.int32 and tgt.tolist() == [-1, 7, 0]
    # scalar: the same number at every phoneme of every utterance, neutral past the utterance's end
    assert (pc[0, :5] == 1.5).all() and (pc[0, 5:] == 1.0).all() and (pc[1, :3] == 1.5).all() and (pc[2] == 1.5).all()
    # per utterance
    assert (ec[0, :5] == np.float32(0.9)).all() and (ec[1, :3] == 1.0).all() and (ec[2] == np.float32(1.1)).all() and (ec[0, 5:] == 1.0).all()
    # per phoneme, None = neutral, scalar entry
    assert np.array_equal(dc[0, :5], np.linspace(1, 2, 5).astype(np.float32)) and (dc[1] == 1.0).all() and (dc[2] == 0.5).all()
    # NaN = not set; padding has 0 and value 0
    assert ph.tolist() == [[0] * 8, [1, 0, 1] + [0] * 5, [0] * 8]
    assert pv[1, :3].tolist() == [1.0, 0.0, 3.0] and not pv[0].any()
    assert not eh.any() and not ev.any()
    assert dh.tolist() == [[0, 1, 0, 1, 0, 0, 0, 0], [0] * 8, [1] * 8]
    assert dv[0, :5].tolist() == [0.0, 4.0, 0.0, 0.0, 0.0] and (dv[2] == 2.0).all()
    # a sub-batch in another order, padded to another bucket
    sub = p.padded([2, 0], 16)
    assert sub[0].shape == (2, 16) and sub[-1].tolist() == [0, -1] and (sub[6][0, :8] == 0.5).all() and (sub[6][0, 8:] == 1.0).all()
    assert np.array_equal(sub[6][1, :5], dc[0, :5])
    # a NaN in a control is "not set" too: neutral
    q = batching.plan_prosody((3,), p_control=[[2.0, nan, 0.5]])
    assert q.padded([0], 8)[0][0, :3].tolist() == [2.0, 1.0, 0.5]
    # what the scalar route can express, and what it cannot
    assert p.plain(1) is None and p.plain(0) is None and p.plain(2) is None
    r = batching.plan_prosody(LENS, p_control=[np.full(5, 1.5), 1.0, 1.0], d_control=0.9, pitch=[None, 2.0, None])
    assert r.plain(0) == (1.5, 1.0, np.float32(0.9)) and r.plain(1) is None and r.plain(2) == (1.0, 1.0, np.float32(0.9))
    # integer targets as one number for all
    assert batching.plan_prosody(LENS, target_frames=40).target.tolist() == [40, 40, 40]
    assert batching.plan_prosody(LENS, target_frames=np.int64(3)).target.tolist() == [3, 3, 3]


def test_which_calls_take_the_new_route():
    w = batching.wants_rows
    none3 = (None, None, None)
    assert not w(3, (1.0, 1.5, 0.9), none3, None)
    assert not w(3, ([0.9, 1.0, 1.1], np.array([1.0, 1.0, 1.0], np.float32), (1, 2, 3)), none3, None)
    assert not w(3, ([1.0, 1.0], 1.0, 1.0), none3, None)              # a wrong count stays with the existing route's own error
    assert w(3, ([np.ones(5), 1.0, None], 1.0, 1.0), none3, None)
    assert w(3, (np.ones((3, 8)), 1.0, 1.0), none3, None)
    assert w(2, ([np.ones(17), np.ones(48)], 1.0, 1.0), none3, None)     # ragged: no rectangular array
    assert w(3, (1.0, 1.0, 1.0), (None, None, 2.0), None)
    assert w(3, (1.0, 1.0, 1.0), none3, 100)
    assert w(3, (1.0, 1.0, 1.0), none3, [None, None, None])


@pytest.mark.parametrize("kw, match", [
    (dict(p_control=[np.ones(4), 1.0, 1.0]), r"p_control\[0\].*5 values"),
    (dict(e_control=[1.0, 1.0]), r"e_control.*3 entries"),
    (dict(d_control=[1.0, np.ones((2, 3)), 1.0]), r"d_control\[1\]"),
    (dict(pitch=[None, None, np.ones(9)]), r"pitch\[2\].*8 values"),
    (dict(energy=[None, [1.0, float("inf"), 2.0], None]), r"energy\[1\].*finite"),
    (dict(pitch=[float("-inf"), None, None]), r"pitch\[0\].*finite"),
    (dict(p_control=[1.0, [1.0, float("inf"), 1.0], 1.0]), r"p_control\[1\].*finite"),
    (dict(durations=[None, [1.0, -1.0, 2.0], None]), r"durations\[1\].*>= 0"),
    (dict(durations=[None, None, float("inf")]), r"durations\[2\].*finite"),
    (dict(durations=[np.ones(5), np.ones(3)]), r"durations.*3 entries"),
    (dict(durations=[None, "abc", None]), r"durations\[1\]"),
    (dict(target_frames=[10, -1, None]), r"target_frames\[1\]"),
    (dict(target_frames=[10, 2.5, None]), r"target_frames\[1\]"),
    (dict(target_frames=float("nan")), r"target_frames\[0\]"),
    (dict(target_frames=[1, 2]), r"target_frames.*3 entries"),
])
def test_every_validation_error_names_argument_and_utterance(kw, match):
    with pytest.raises(ValueError, match=match):
        batching.plan_prosody(LENS, **kw)


def test_front_key_depends_on_the_shape_alone():
    a = batching.plan_prosody(LENS, p_control=[np.linspace(0.5, 2, 5), 1.0, 1.0])
    b = batching.plan_prosody(LENS, durations=[None, 3.0, None], pitch=2.5, target_frames=[None, 90, 4])
    assert [x.shape for x in a.padded([0, 1, 2], 8)] == [x.shape for x in b.padded([0, 1, 2], 8)]
    assert [x.dtype for x in a.padded([0, 1, 2], 8)] == [x.dtype for x in b.padded([0, 1, 2], 8)]
    assert batching.rows_key(3, 8) == ("front", 3, 8, "rows") != batching.front_key(3, 8)
    rng = np.random.RandomState(0)
    plan = batching.plan_texts([rng.randint(1, 207, size=n) for n in LENS], 1000)
    assert plan.key == ("front", 3, 8)                     # the existing route's key is as before


# ------------------------------------------------------------------------------------------------ the oracle's semantics
@pytest.mark.parametrize("L", [17, 48])
def test_oracle_broadcasts_control_tensors_per_phoneme(L):
    cfg, sd = oracle_weights()
    g = torch.Generator().manual_seed(100 + L)
    ids = torch.randint(1, 207, (1, L), generator=g)
    args = (sd, cfg.model_config, torch.tensor([5]), ids, torch.tensor([L]), L)
    with torch.no_grad():
        scalar = ofs2.fs2_forward(*args, p_control=1.5, e_control=0.8, d_control=1.1)
        rows = ofs2.fs2_forward(*args, p_control=torch.full((1, L), 1.5), e_control=torch.full((1, L), 0.8), d_control=torch.full((1, L), 1.1))
        for k in (0, 1, 2, 3, 4, 8, 9):         # constant rows: the scalar run
            assert torch.equal(scalar[k], rows[k]), k
        pc, ec, dc = (torch.rand(1, L, generator=g) * 1.5 + 0.25 for _ in range(3))
        one = ofs2.fs2_forward(*args)
        var = ofs2.fs2_forward(*args, p_control=pc, e_control=ec, d_control=dc)
    assert torch.equal(var[3], one[3])                           # the duration predictor reads no control
    assert torch.equal(var[1], one[1] * pc)                      # pitch_pred * pc, elementwise
    assert torch.equal(var[4], torch.clamp(torch.round(torch.exp(one[3]) - 1) * dc, min=0))
    assert int(var[8][0]) == int(var[4].long().sum())          # LengthRegulator truncates
    # explicit values mixed with the model's own predictions: set positions are used as given
    has = torch.rand(1, L, generator=g) < 0.4
    mixed = torch.where(has, torch.full((1, L), 2.25), var[1])
    with torch.no_grad():
        tf = ofs2.fs2_forward(*args, pitches_raw=mixed, e_control=ec, d_control=dc)
        same = ofs2.fs2_forward(*args, pitches_raw=var[1], e_control=ec, d_control=dc)
    assert torch.equal(same[2], var[2]) and torch.equal(same[9], var[9])     # feeding the scaled pitch back changes nothing
    assert bool(has.any()) and not torch.equal(tf[2], var[2])                # the energy predictor sees the set values


# ------------------------------------------------------------------------------------------------ the fit rule
def test_fit_rule_hand_worked_cases():
    f = lambda v, has, t: fit_rule(v, has, t).tolist()
    no = [False] * 8
    assert f([2.7, 0.3], no[:2], -1) == [np.float32(2.7), np.float32(0.3)]          # no target: untouched, fractions and all
    assert f([1, 1, 1], no[:3], 4) == [2, 1, 1]                  # q = 4/3 each: the one missing frame goes to the lowest l
    assert f([2, 2, 2, 2], no[:4], 6) == [2, 2, 1, 1]            # ties in the fractional part: lower l first
    assert f([3, 1], no[:2], 6) == [5, 1]                        # q = 4.5, 1.5: tie -> l = 0
    assert f([0, 2, 0, 1], no[:4], 2) == [0, 1, 0, 1]            # v = 0 stays 0; 4/3 -> 1, 2/3 -> 0 + the missing frame
    assert f([2, 3], no[:2], 0) == [0, 0]                        # target 0
    assert f([2, 3, 4], no[:3], 1) == [0, 0, 1]                  # a target below the number of non-zero phonemes: q = 2/9, 3/9, 4/9
    assert f([0, 0, 3], [False, False, True], 10) == [0, 0, 3]   # S = 0: the free stay 0, F frames
    assert f([5, 2], [True, False], 3) == [5, 0]                 # target < F: the explicit durations win
    assert f([5, 2], [True, False], 5) == [5, 0]
    assert f([5.9, 2], [True, False], 9) == [5, 4]               # a fixed phoneme keeps trunc(v)
    assert f([2.7, 1.2], [True, True], 9) == [2, 1]              # all fixed
    assert f([2.7, 0.9, 0.9], no[:3], 9) == [5, 2, 2]            # fractional v (a control of 0.9): q = 5.4, 1.8, 1.8 -> 5, 1, 1 + two frames
    rng = np.random.RandomState(3)
    for n, t in ((1, 5), (7, 100), (257, 40), (1000, 8000), (1000, 3)):
        v = np.round(rng.rand(n) * 6).astype(np.float32) * np.float32(0.9)
        has = rng.rand(n) < 0.2
        out = fit_rule(v, has, t)
        F, free = np.trunc(v[has].astype(np.float64)).sum(), ~has & (v > 0)
        assert out.sum() == (max(t, F) if free.any() else F), (n, t)
        assert (out == np.floor(out)).all() and (out >= 0).all() and (out[~has & (v == 0)] == 0).all()
