"""CPU: the HiFi-GAN generator's per-stage plan (`Generator._plan()`, tts_king_amd/hifigan.py) — built from the configuration, the
storage type and the toggle attributes alone, on a generator whose weights are on no device (the built library's host predicates
only): `stage_routes()` over the 32 settings of the route toggles for V1, V2 and V3 equals the table recorded from the commit named in
tests/golden/hifi_route_launches.json; the plan is rebuilt exactly when a toggle or the storage type changes; a configuration the
conv-by-conv route cannot average is refused by the plan builder."""
import copy
import json
import os

import pytest
import torch

from tests.hifi_generic_ref import v2_config
from tests.hifi_routes_util import GRID, route_table

CHANGED = {"window_conv": False, "conv_pair": False, "conv_pair_small": False, "pair_ws": False, "pair_ws_min_tiles": 1, "fused": False,
           "stream_upsample": False, "window_upsample": False, "loop_upsample": False, "mrf_fused": False, "resblock2_fused": False,
           "act_dtype": torch.bfloat16}


def test_stage_routes_over_the_toggle_grid_are_the_recorded_ones(cfg, golden_dir):
    with open(os.path.join(golden_dir, "hifi_route_launches.json")) as f:
        golden = json.load(f)
    assert tuple(golden["grid"]) == GRID
    got = route_table(cfg)
    assert sorted(got) == sorted(golden["route_table"]) == ["v1", "v2", "v3"]
    for name, want in golden["route_table"].items():
        assert len(want) == 32
        for bits, routes in want.items():
            assert got[name][bits] == routes, (name, dict(zip(GRID, bits)), got[name][bits], routes)


def test_v1_at_defaults_plans_the_shipped_kernels(cfg):
    from tts_king_amd.hifigan import Generator
    gen = Generator(cfg.hifi)
    gen.window_upsample = True                         # (its default reads an environment switch)
    plan = gen._plan()
    assert plan.conv_pre == "win" and plan.conv_post == "fused"
    assert [s.ups for s in plan.stages] == ["win", "loop", "win", "stream"]
    assert [s.route for s in plan.stages] == ["pair", "pair", "pair", "mrf32_post"]
    assert [s.fused_for for s in plan.stages] == [(), (), (3,), ()] and not any(s.act_copy for s in plan.stages)
    assert [s.nxt_slope for s in plan.stages] == [0.1, 0.1, 0.1, 0.01]
    gen.fused = False
    plan = gen._plan()
    assert [(s.route, s.gemm, s.act_copy, s.ups) for s in plan.stages[2:]] == [("gemm", "lockstep", True, "gemm")] * 2 and plan.conv_post == "stream"
    gen.fused, gen.conv_pair = True, False
    assert [(s.route, s.gemm) for s in gen._plan().stages[:2]] == [("gemm", "lockstep"), ("gemm", "window")]


@pytest.mark.parametrize("name", list(CHANGED))
def test_plan_is_rebuilt_when_a_toggle_changes_and_only_then(cfg, name):
    from tts_king_amd.hifigan import Generator
    gen = Generator(cfg.hifi)
    gen.window_upsample = True
    plan = gen._plan()
    assert gen._plan() is plan and gen.stage_routes() == gen.stage_routes() and gen._plan() is plan
    keep = getattr(gen, name)
    assert keep != CHANGED[name]
    setattr(gen, name, CHANGED[name])
    other = gen._plan()
    assert other is not plan and other.key != plan.key and gen._plan() is other
    setattr(gen, name, keep)
    assert gen._plan().key == plan.key


def test_two_mrf_kernel_sizes_conv_by_conv_are_refused_by_the_plan_builder(cfg):
    from tts_king_amd.hifigan import Generator
    c = v2_config(cfg)
    c.hifi["resblock_kernel_sizes"], c.hifi["resblock_dilation_sizes"] = [3, 7], [[1, 3, 5], [1, 3, 5]]
    gen = Generator(copy.deepcopy(c.hifi))
    with pytest.raises(NotImplementedError) as e:
        gen._plan()
    assert "stage 2" in str(e.value)
    assert gen.stage_routes() == ["pair", "fused", "gemm", "gemm"]            # the routes themselves can still be asked for
