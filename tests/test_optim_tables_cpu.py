"""CPU: `ops.optim_tables`, the host side of the optimizer step's three tables (include/ttsk.h, ttsk_optim_step): ranges, packed items
with their first tiles, and the gaps = the ranges minus the items.  The expected tables are worked out by hand for one layout: a
131,072-float buffer with item A, storage (32, 1, 256) = one 32 x 256 tile = 8,192 floats at offset 64 with both packs, and item B,
storage (64, 3, 512) = 3 taps x 2 row tiles x 2 column blocks = 12 tiles = 98,304 floats at offset 16,704 with the transposed pack only.
The device side of the same layout is tests/test_adapt_optim_gpu.py."""
import torch

from tts_king_amd import lib as L
from tts_king_amd import ops

BF = torch.bfloat16
N = 131072
A_OFF, A_SHAPE = 64, (32, 1, 256)          # [64, 8256)
B_OFF, B_SHAPE = 16704, (64, 3, 512)       # [16704, 115008)


def _packs():
    return {(k, tr): torch.empty(ops.win_pack_numel(*shp, tr), dtype=BF) for k, shp, tr in (("A", A_SHAPE, False), ("A", A_SHAPE, True), ("B", B_SHAPE, True))}


def _items(pk):
    return [(B_OFF, B_SHAPE, None, pk["B", True]), (A_OFF, A_SHAPE, pk["A", False], pk["A", True])]      # unsorted on purpose


def _decode(t, n):
    arr = (L.AdamItem * n).from_buffer_copy(t.numpy().tobytes())
    return [(it.off, it.pack, it.pack_t, it.Cs, it.K, it.Ds, it.tile0) for it in arr]


def test_one_full_range_with_items():
    pk = _packs()
    t = ops.optim_tables([(0, N)], _items(pk), "cpu")
    assert t["ranges"].tolist() == [0, N, 0] and t["n_ranges"] == 1 and t["range_floats"] == N and t["end"] == N
    assert t["n_items"] == 2 and t["n_tiles"] == 1 + 12
    assert _decode(t["items"], 2) == [(A_OFF, pk["A", False].data_ptr(), pk["A", True].data_ptr(), 32, 1, 256, 0),
                                      (B_OFF, None, pk["B", True].data_ptr(), 64, 3, 512, 1)]
    # gaps: before A, between A and B, behind B; third column = groups of four floats in the gaps before
    assert t["n_gaps"] == 3 and t["gaps"].tolist() == [0, 64, 0, 8256, 16704, 16, 115008, N, 16 + 2112]
    assert t["gap_floats"] == 64 + 8448 + 16064 == N - 13 * 8192


def test_items_in_two_ranges():
    pk = _packs()
    ranges = [(16640, 120000), (0, 8320)]                                 # unsorted on purpose
    t = ops.optim_tables(ranges, _items(pk), "cpu")
    assert t["ranges"].tolist() == [0, 8320, 0, 16640, 120000, 2080] and t["n_ranges"] == 2 and t["end"] == 120000
    assert t["range_floats"] == 8320 + 103360
    assert [it[0] for it in _decode(t["items"], 2)] == [A_OFF, B_OFF] and [it[6] for it in _decode(t["items"], 2)] == [0, 1]
    assert t["n_gaps"] == 4 and t["gaps"].tolist() == [0, 64, 0, 8256, 8320, 16, 16640, 16704, 32, 115008, 120000, 48]
    assert t["gap_floats"] == 64 + 64 + 64 + 4992 == t["range_floats"] - 13 * 8192
    # an item at the very start and the very end of its range: no empty gaps
    t = ops.optim_tables([(A_OFF, A_OFF + 8192), (B_OFF, B_OFF + 98304)], _items(pk), "cpu")
    assert t["n_gaps"] == 0 and t["gap_floats"] == 0 and t["n_tiles"] == 13 and t["range_floats"] == 13 * 8192


def test_no_items():
    t = ops.optim_tables([(0, 64), (128, 136)], [], "cpu")
    assert t["ranges"].tolist() == [0, 64, 0, 128, 136, 16] and t["range_floats"] == 72 and t["end"] == 136
    assert t["items"] is None and t["gaps"] is None and (t["n_items"], t["n_tiles"], t["n_gaps"], t["gap_floats"]) == (0, 0, 0, 0)
    assert ops.optim_tables([], [], "cpu")["n_ranges"] == 0


def test_what_cannot_be_tabled_returns_none():
    pk = _packs()
    a = (A_OFF, A_SHAPE, pk["A", False], pk["A", True])
    assert ops.optim_tables([(0, N)], [a], "cpu") is not None
    assert ops.optim_tables([(0, 8192)], [a], "cpu") is None                       # the item straddles the range end (8256 > 8192)
    assert ops.optim_tables([(128, N)], [a], "cpu") is None                        # ... the range start
    assert ops.optim_tables([(0, 4096), (4096 + 8, N)], [a], "cpu") is None        # ... a frozen stretch
    assert ops.optim_tables([(0, 32), (16640, N)], [a], "cpu") is None             # an item outside every range
    assert ops.optim_tables([(0, N)], [(A_OFF, (48, 1, 256), None, None)], "cpu") is None      # Cs % 32
    assert ops.optim_tables([(0, N)], [(A_OFF, (32, 1, 128), None, None)], "cpu") is None      # Ds % 256
    assert ops.optim_tables([(0, N)], [(A_OFF + 2, A_SHAPE, None, None)], "cpu") is None       # offset not a multiple of four
    assert ops.optim_tables([(0, N)], [a, (A_OFF + 4096, A_SHAPE, None, None)], "cpu") is None  # overlapping items
    assert ops.optim_tables([(0, 64), (32, 128)], [], "cpu") is None               # overlapping ranges
    assert ops.optim_tables([(0, 66)], [], "cpu") is None                          # not multiples of four floats
    assert ops.optim_tables([(2, 66)], [], "cpu") is None
