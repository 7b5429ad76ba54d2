"""GPU: a HiFi-GAN generator forward launches exactly what tests/golden/hifi_route_launches.json records — every launch with its
integer and float arguments, in order — for V1 under each kernel-family toggle, V2, V3 and the per-row-length route
(tests/hifi_routes_util.py; tools/make_goldens_hifi_routes.py wrote the golden on an MI355X from the commit it names), and its
waveform is that commit's bit for bit.  The waveform tests compare values within a tolerance; a stage that moves to another kernel
family keeps them green."""
import json
import os

import pytest
import torch

from tests.hifi_routes_util import CASES, Recorder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorder(cfg):
    return Recorder(cfg)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "hifi_route_launches.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_is_the_recorded_one(recorder, golden, name):
    want = golden["cases"][name]
    got = recorder.record(name)
    print("%s: routes %s, short_rows %s, %s (golden of %s: %s)" % (
        name, got["routes"], got["short_rows"], got.get("raises") or "%d launches, waveform sha256 %s" % (len(got["launches"]), got["wav_sha256"]),
        golden["commit"][:7], want.get("raises") or want["wav_sha256"]))
    assert got["routes"] == want["routes"] and got["short_rows"] == want["short_rows"]
    assert got.get("raises") == want.get("raises")
    if "raises" in want:
        return
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        assert g == w, "launch %d of %d: %s, recorded %s" % (i, len(want["launches"]), g, w)
    assert len(got["launches"]) == len(want["launches"])
    assert want["wav_sha256"] is not None and got["wav_sha256"] == want["wav_sha256"]


def test_a_flipped_toggle_is_picked_up_by_the_next_forward(recorder, golden):
    """`window_upsample`, then `act_dtype`, flipped on ONE generator between two forwards: the next forward launches what a generator
    built with that setting launches (the recorded cases), with no cache poke; with nothing changed, `_prepare()` hands back the very
    same pack objects."""
    gen = recorder.gen("v1")

    def launches():
        recorder.forward(gen)                            # packing is not part of a forward
        log = []
        recorder.forward(gen, log=log)
        return log

    base = launches()
    assert base == golden["cases"]["v1"]["launches"]
    pk = gen._prepare()
    assert gen._prepare() is pk
    recorder.forward(gen)
    assert gen._prepare() is pk
    gen.window_upsample = False
    off = launches()
    assert off == golden["cases"]["v1_no_window_upsample"]["launches"] and off != base
    assert gen._prepare() is not pk
    gen.window_upsample = True
    assert launches() == base
    gen.act_dtype = torch.bfloat16
    bf = launches()
    assert bf == golden["cases"]["v1_bf16"]["launches"] and bf != base
