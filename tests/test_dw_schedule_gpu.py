"""GPU: the FastSpeech2 backward issues its deferred weight-gradient work (grouped dW GEMMs, dwconv / dwgemm problems, split-K
reducers, column sums) and announces its gradient buckets exactly as recorded in tests/golden/dw_schedule_launches.json — every
launch of the step with its stream, its item count and its grid cap, in order (tests/dw_schedule_util.py;
tools/make_goldens_dw_schedule.py wrote the golden on an MI355X from the commit it names).  The gradient tests compare values; a
launch that moves to another stream or behind a bucket's announcement leaves the values of a one-GPU run alone."""
import json
import os

import pytest

from tests.dw_schedule_util import CONFIGS, Recorder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorder(cfg):
    return Recorder(cfg)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "dw_schedule_launches.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_launch_sequence_is_the_recorded_one(recorder, golden, name):
    want = golden["configs"][name]
    got = recorder.record(name)
    print("%s: %d launches, counts %s, %d trace entries, gradient sha256 %s (golden of %s: %s)" % (
        name, len(got["launches"]), got["counts"], len(got["trace"]), got["grad_sha256"], golden["commit"][:7], want["grad_sha256"]))
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        assert g == w, "launch %d of %d: %s, recorded %s" % (i, len(want["launches"]), g, w)
    assert len(got["launches"]) == len(want["launches"])
    assert got["counts"] == want["counts"]
    assert got["trace"] == want["trace"]
    if want["grad_sha256"] is not None:
        assert got["grad_sha256"] == want["grad_sha256"]
