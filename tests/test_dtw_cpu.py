"""CPU: the fp64 restatement of ttsk_dtw_align (tests/dtw_ref.py) against brute force and against a known warp, the host-side
refusals of `ops.dtw_align` and of the library entry point, and the argument handling around alignment that needs no device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dtw_ref
from tts_king_amd import lib, ops, preprocess
from tts_king_amd.lib import TtskError


@pytest.mark.parametrize("Tx", range(1, 6))
@pytest.mark.parametrize("Ty", range(1, 6))
def test_restatement_against_all_monotone_paths(Tx, Ty):
    """Integer features in {-2..2}, C = 3: every cost is an exact integer, ties abound.  Same optimal cost, and the path is the one
    the tie rule picks among the optimal ones."""
    rng = np.random.default_rng(100 * Tx + Ty)
    for _ in range(6):
        x = rng.integers(-2, 3, size=(Tx, 3)).astype(np.float64)
        y = rng.integers(-2, 3, size=(Ty, 3)).astype(np.float64)
        A, path, path_x, _ = dtw_ref.dtw(x, y)
        best, paths = dtw_ref.brute_force(x, y)
        assert A[-1, -1] == best
        assert dtw_ref.path_cost(x, y, path) == best
        assert path == dtw_ref.tie_rule_pick(paths)
        assert path_x.tolist() == [max(i for i, jj in path if jj == j) for j in range(Ty)]
        assert dtw_ref.path_from_path_x(path_x, Tx) == path


def test_warp_property():
    rng = np.random.default_rng(5)
    Tx, Ty = 40, 71
    x = rng.standard_normal((Tx, 4))
    w = dtw_ref.make_warp(rng, Tx, Ty)
    assert w[0] == 0 and w[-1] == Tx - 1
    x_seg = [3, 0, 10, 7, 0, 20]
    A, path, path_x, dur = dtw_ref.dtw(x, x[w], x_seg)
    assert A[-1, -1] == 0.0 and path_x.tolist() == w.tolist()
    assert dur.tolist() == dtw_ref.histogram_over_segments(w, x_seg).tolist() and dur.sum() == Ty and dur[1] == 0 and dur[4] == 0


def test_path_cost_refuses_a_broken_path():
    x = np.zeros((3, 1))
    for bad in ([(0, 0), (2, 2)], [(0, 0), (1, 1)], [(0, 0), (1, 0), (0, 1), (2, 2)], [(0, 0), (0, 0), (1, 1), (2, 2)]):
        with pytest.raises(AssertionError):
            dtw_ref.path_cost(x, x, bad)


def test_restatement_is_quick_at_the_largest_test_shape():
    import time
    rng = np.random.default_rng(1)
    x, y = rng.integers(-2, 3, size=(1100, 2)).astype(np.float64), rng.integers(-2, 3, size=(1030, 2)).astype(np.float64)
    t0 = time.perf_counter()
    A, path, path_x, _ = dtw_ref.dtw(x, y)
    print("dtw_ref.dtw at 1100 x 1030: %.3f s" % (time.perf_counter() - t0))
    assert dtw_ref.path_cost(x, y, path) == A[-1, -1]


def test_ops_dtw_align_refuses_on_the_host():
    """Every refusal comes before any device call: the tensors are on the CPU, and the message names the argument."""
    f = lambda *s: torch.zeros(*s)
    with pytest.raises(TtskError, match="C = 129"):
        ops.dtw_align(f(1, 4, 129), f(1, 4, 129))
    with pytest.raises(TtskError, match="x has 2049 frames"):
        ops.dtw_align(f(1, 2049, 2), f(1, 4, 2))
    with pytest.raises(TtskError, match="y has 2049 frames"):
        ops.dtw_align(f(1, 4, 2), f(1, 2049, 2))
    with pytest.raises(TtskError, match="x must be a contiguous"):
        ops.dtw_align(f(1, 4, 2).double(), f(1, 4, 2))
    with pytest.raises(TtskError, match="y must be a contiguous"):
        ops.dtw_align(f(1, 4, 2), f(1, 2, 4).transpose(1, 2))
    with pytest.raises(TtskError, match="y_lens must be"):
        ops.dtw_align(f(1, 4, 2), f(1, 4, 2), None, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TtskError, match="x_seg has 1025 phonemes"):
        ops.dtw_align(f(1, 4, 2), f(1, 4, 2), x_seg=torch.zeros(1, 1025, dtype=torch.int32))
    with pytest.raises(TtskError, match="x_seg must be"):
        ops.dtw_align(f(1, 4, 2), f(1, 4, 2), x_seg=torch.zeros(1, 8, dtype=torch.int64))
    with pytest.raises(TtskError, match="no CPU path"):                     # all checks passed: only then the device is asked for
        ops.dtw_align(f(1, 4, 2), f(1, 4, 2))


def test_library_refuses_sizes_past_its_limits_before_any_launch():
    L = lib.load()
    buf = (C.c_ubyte * (4096 + 16))()
    p = (C.addressof(buf) + 15) & ~15
    call = lambda B, ldx, ldy, Cc, ldL=0, seg=None, ws=p, nbytes=4096: L.ttsk_dtw_align(p, p, None, None, B, ldx, ldy, Cc, seg, None, ldL, ws, nbytes,
                                                                                      p, p, p, seg, None)
    for args, word in (((1, 4, 4, 129), b"C 129"), ((1, 4, 4, 0), b"C 0"), ((1, 2049, 4, 2), b"ldx 2049"), ((1, 4, 2049, 2), b"ldy 2049"),
                       ((-1, 4, 4, 2), b"B -1"), ((1, 4, 4, 2, 1025, p), b"ldL 1025"), ((1, 4, 4, 2, 0, None, None), b"workspace"),
                       ((1, 4, 4, 2, 0, None, p, 100), b"workspace"), ((1, 4, 4, 2, 0, None, p + 4), b"aligned")):
        assert call(*args) == -1, args
        assert word in L.ttsk_last_error(), (args, L.ttsk_last_error())
    assert call(0, 4, 4, 2) == 0                                             # B = 0 launches nothing
    assert L.ttsk_dtw_workspace_bytes(1, 4, 4) == 5 * 8 * 4 and L.ttsk_dtw_workspace_bytes(0, 4, 4) == 0
    assert L.ttsk_dtw_workspace_bytes(32, 2048, 2048) == 32 * 4096 * 2048 * 5 and L.ttsk_dtw_workspace_bytes(1, 2049, 4) == -1


def test_extract_prosody_wants_exactly_one_of_durations_and_text():
    import tts_king
    tts = tts_king.TTSKing.__new__(tts_king.TTSKing)          # no model, no device: the check comes first
    wav = np.zeros(1000)
    with pytest.raises(ValueError, match="neither"):
        tts.extract_prosody(wav)
    with pytest.raises(ValueError, match="both"):
        tts.extract_prosody(wav, [3, 4], text="{R A}")


def test_lab_phonemes_and_the_speaker_used_for_alignment():
    from tts_king_amd.text import sequence_to_text, text_to_sequence
    ids = preprocess.lab_phonemes("{R A B O0 T A}\n")
    assert ids.tolist() == text_to_sequence("{R A B O0 T A}", []) and len(ids) == 6
    assert sequence_to_text(ids.tolist()) == "{R A B O0 T A}"
    assert preprocess.lab_phonemes("plain words") is None
    assert preprocess.lab_phonemes("plain words", g2p=lambda s: [[5, 6, 7]]).tolist() == [5, 6, 7]
    known = ["anna", "boris"]
    assert preprocess.align_speaker("boris", known) == "boris"
    assert preprocess.align_speaker("carl", known) == "anna"
    assert preprocess.align_speaker("carl", known, "boris") == "boris"
