"""CPU: FastSpeech2's kernel plan (tts_king_amd/fs2_plan.py: `build_plan`, `FastSpeech2.plan`, `routes()`) -- built from the
dimensions and the five toggles alone, with the model on no device (the built library's host predicates only): its packs are the ones
recorded from the commit named in tests/golden/fs2_route_launches.json; `routes()` names the shipped kernels for the shipped
configuration (hand-written from the launch counts of tests/test_fs2_configs_gpu.py: ROUTE) and, for each configuration of
tests/fs2_configs.py, the branch its `selects` text claims; the plan is rebuilt exactly when a toggle changes; and over every
configuration and toggle setting a block names the "pre" hand-over exactly when the block in front of it consumes it."""
import json
import os

import pytest

from tests import fs2_configs as FC
from tests.fs2_routes_util import CASES, TOGGLES, build_model, config, toggle_grid

NAMES = ["shipped"] + list(FC.CONFIGS)
_MODELS = {}


def model(cfg, name):
    """One model per configuration on the CPU, toggles at their defaults."""
    if name not in _MODELS:
        _MODELS[name] = build_model(config(cfg, name), {}, device="cpu")
    return _MODELS[name]


def plan_of(cfg, name, toggles):
    from tts_king_amd import fs2_plan
    m = model(cfg, name)
    return fs2_plan.build_plan(m._dims, fs2_plan.Toggles(**dict(m._toggles, **toggles)))


def stacks(r):
    """site -> route names over both stacks' blocks."""
    return {site: r["encoder"][site] + r["decoder"][site] for site in r["encoder"]}


@pytest.mark.parametrize("name", NAMES)
def test_plan_builds_with_the_model_on_no_device(cfg, name):
    m = model(cfg, name)
    assert m.device.type == "cpu" and m._w1_packed is None
    plan = m.plan
    assert len(plan.encoder) == m.n_enc and len(plan.decoder) == m.n_dec and len(plan.postnet) == 5
    assert m.plan is plan and m.routes() == m.routes() and m.plan is plan


@pytest.mark.parametrize("case", [n for n, (_, t) in CASES.items() if not t] + ["no_postnet_ends_win"])
def test_packs_are_the_recorded_ones(cfg, golden_dir, case):
    with open(os.path.join(golden_dir, "fs2_route_launches.json")) as f:
        want = json.load(f)["cases"][case]["packs"]
    name, toggles = CASES[case]
    m = model(cfg, name)
    got = sorted([p.tag, p.key, m.pack_numel(p)] for p in plan_of(cfg, name, toggles).packs)
    assert len(want) > 0 and got == want


def test_shipped_configuration_plans_the_shipped_kernels(cfg):
    r = model(cfg, "shipped").routes()
    for name, n in (("encoder", 4), ("decoder", 6)):
        s = r[name]
        assert s["w1"] == ["ffn"] * n and s["attn"] == ["flash"] * n and s["fc_ln"] == ["win_ln"] * n
        assert s["w2_ln"] == ["win_ln_proj"] * (n - 1) + ["win_ln"] and s["qkv"] == ["win"] + ["chained"] * (n - 1)
        assert s["w2_bwd"] == ["ln_proj"] * n and s["fc_bwd"] == ["ln_proj"] * n and s["fc_delta"] == [True] * n
        assert s["qkv_dx"] == ["qkv_dx"] + ["pre"] * (n - 1)
        assert s["w1_dx"] == ["win_split"] * n and s["w1_dw"] == ["dwconv"] * n
    assert r["mel_linear"] == {"train": "win_dual", "eval": "gemm", "dx": "win"}
    assert r["postnet"]["conv"] == ["win_stats"] * 5 and r["postnet"]["conv_eval"] == ["win"] * 5 and r["postnet"]["bn"] == ["slab"] * 5
    assert r["postnet"]["dx"] == ["win_resid"] + ["win_bnb"] * 4


def test_each_configuration_plans_the_branch_it_was_chosen_for(cfg):
    s = stacks(model(cfg, "heads_1_4").routes())
    assert s["attn"] == ["softmax"] * 10 and s["fc_delta"] == [False] * 10 and s["w1"] == ["ffn"] * 10
    s = stacks(model(cfg, "d512").routes())
    assert s["attn"] == ["flash"] * 10 and s["fc_ln"] == s["w2_ln"] == ["split"] * 10 and s["w1"] == ["win"] * 10
    assert s["qkv"] == ["win"] * 10 and s["w1_dx"] == ["win_split"] * 10 and s["w1_dw"] == ["dwconv"] * 10
    for site in ("w2_bwd", "fc_bwd", "qkv_dx"):
        assert "ln_proj" not in s[site] and "qkv_dx" not in s[site] and "pre" not in s[site], site
    s = stacks(model(cfg, "ffn_k3").routes())
    assert s["w2_ln"] == ["split"] * 10 and s["fc_ln"] == ["win_ln"] * 10 and s["w1"] == ["ffn"] * 10
    assert s["w1_dw"] == ["queue"] * 10 and s["w2_bwd"] == ["gemm"] * 10 and "pre" not in s["qkv_dx"]
    r = model(cfg, "mel40_layers_1_2").routes()
    assert r["mel_linear"] == {"train": "gemm", "eval": "gemm", "dx": "gemm"}
    assert r["postnet"]["conv"] == ["gemm", "win_stats", "win_stats", "win_stats", "gemm"] and r["postnet"]["bn"] == ["slab"] * 5
    assert r["postnet"]["dx"] == ["gemm", "win_bnb", "win_bnb", "win_bnb", "gemm"]
    assert r["encoder"]["qkv"] == ["win"] and r["encoder"]["w2_ln"] == ["win_ln"] and r["decoder"]["qkv"] == ["win", "chained"]
    for name in ("pred512", "short_table"):
        assert model(cfg, name).routes() == model(cfg, "shipped").routes()


@pytest.mark.parametrize("name", TOGGLES)
def test_plan_is_rebuilt_when_a_toggle_changes_and_only_then(cfg, name):
    m = build_model(config(cfg, "shipped"), {}, device="cpu")
    plan = m.plan
    assert m.plan is plan and m.routes() == m.routes() and m.plan is plan
    setattr(m, name, getattr(m, name))                  # the same value: nothing to rebuild
    assert m.plan is plan
    keep = getattr(m, name)
    setattr(m, name, not keep)
    other = m.plan
    assert getattr(m, name) is (not keep) and other is not plan and other != plan and m.plan is other
    setattr(m, name, keep)
    assert m.plan == plan


@pytest.mark.parametrize("name", NAMES)
def test_pre_hand_over_is_named_exactly_when_the_block_in_front_consumes_it(cfg, name):
    """A block's `qkv_dx` "pre" hands the block in front (dqkv, the transposed q|k|v pack, residual) instead of a gradient; only that
    block's `w2_bwd` "ln_proj" can take it.  Over the 32 toggle settings."""
    seen = set()
    for toggles in toggle_grid():
        plan = plan_of(cfg, name, toggles)
        tags = {p.tag for p in plan.packs}
        for blocks in (plan.encoder, plan.decoder):
            assert blocks[0].qkv_dx in ("qkv_dx", "gemm")
            for front, b in zip(blocks, blocks[1:]):
                assert b.qkv_dx in ("pre", "win_split", "gemm_raw")
                assert (b.qkv_dx == "pre") == (front.w2_bwd == "ln_proj" and "qkvT" in tags), (toggles, front, b)
                assert (b.qkv == "chained") == (front.w2_ln == "win_ln_proj")
                seen.add(b.qkv_dx)
    assert ("pre" in seen) == (name in ("shipped", "heads_1_4", "pred512", "mel40_layers_1_2", "short_table"))
