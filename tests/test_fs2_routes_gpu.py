"""GPU: FastSpeech2 launches exactly what tests/golden/fs2_route_launches.json records -- every launch of a train step, a teacher-forced
eval forward and the two inference halves with its stream and integer arguments, in order -- for the shipped configuration, the six of
tests/fs2_configs.py and the shipped one under each kernel toggle (tests/fs2_routes_util.py; tools/make_goldens_fs2_routes.py wrote
the golden on an MI355X from the commit it names, the last one that chose kernels where it ran them), and the flat gradient buffer and
the outputs of the three passes are that commit's bit for bit, as are the weight packs it holds and the optimizer's item count.  The
parity tests compare values within a tolerance; a site that moves to another kernel keeps them green."""
import json
import os

import pytest

from tests.fs2_routes_util import CASES, PASSES, Recorder, build_model, config, pack_sizes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorder(cfg):
    return Recorder(cfg)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "fs2_route_launches.json")) as f:
        return json.load(f)


def check(got, want, digests=None):
    """`digests`: the ones to compare (default: all)."""
    for p in PASSES:
        for i, (g, w) in enumerate(zip(got["launches"][p], want["launches"][p])):
            assert g == w, "%s launch %d of %d: %s, recorded %s" % (p, i, len(want["launches"][p]), g, w)
        assert len(got["launches"][p]) == len(want["launches"][p]), p
    assert got["packs"] == want["packs"]
    assert got["adam_items"] == want["adam_items"] and got["repack_after_step"] == want["repack_after_step"]
    for key, w in want["sha256"].items():
        if digests is not None and key not in digests:
            continue
        assert w is not None, (key, want["null_reasons"])        # (the recorded commit gave the same bytes twice everywhere)
        assert got["sha256"][key] == w, key


@pytest.mark.parametrize("name", list(CASES))
def test_launches_and_bits_are_the_recorded_ones(recorder, golden, name):
    want = golden["cases"][name]
    got = recorder.record(name)
    print("%s: %s launches, %d packs, Adam items %s, gradient sha256 %s (golden of %s: %s)" % (
        name, [len(got["launches"][p]) for p in PASSES], len(got["packs"]), got["adam_items"], got["sha256"]["grad"], golden["commit"][:7],
        want["sha256"]["grad"]))
    check(got, want)


def test_a_flipped_toggle_rebuilds_the_packs_and_is_picked_up_by_the_next_step(recorder, golden, cfg):
    """`window_ffn`, then `postnet_ends_win`, cleared and set again on ONE model between steps: the packs and the optimizer's items
    follow at once, and the next step launches and computes what a model built with that setting does (the recorded cases)."""
    m = build_model(config(cfg, "shipped"), {})
    base = pack_sizes(m)
    check(recorder.record("shipped", model=m), golden["cases"]["shipped"])
    plan = m.plan
    m.window_ffn = False
    assert m.plan is not plan and pack_sizes(m) == [] and m._adam_items is None
    # (BatchNorm's running statistics have moved with the steps above: the eval digests are a fresh model's only)
    check(recorder.record("no_window_ffn", model=m), golden["cases"]["no_window_ffn"], digests=("train", "grad"))
    m.window_ffn = True
    assert m.plan == plan and pack_sizes(m) == base
    m.postnet_ends_win = False
    assert pack_sizes(m) == golden["cases"]["no_postnet_ends_win"]["packs"]
    m.postnet_ends_win = True
    assert pack_sizes(m) == base and m._optim_tables["n_items"] == golden["cases"]["shipped"]["adam_items"]
