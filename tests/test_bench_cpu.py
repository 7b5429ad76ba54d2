"""bench.py's ONE line: it must fit the driver's 8 KB stdout tail with both halves of the metric in it, and
`roofline.frac` must follow from the committed rocprofv3 summary under profiles/."""
import glob
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _full_records():
    return sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[5-9]*_bench.json")))


def _worst_case(rec):
    """The same record with everything a multi-GPU / profiled run adds: six bucket sizes, long source strings, unknown switches."""
    r = json.loads(json.dumps(rec))
    r["config"].update({"collective_world_size": 8, "collective_backend": "nccl", "allreduce_bucket_bytes": [25165824] * 6,
                        "allreduces_per_step": 6, "collective_timeout_s": 300.0, "parallelism": "dp8"})
    r["unknown_switches"] = ["TTSK_SOMETHING_NOBODY_READS_%d" % i for i in range(6)]
    if r.get("roofline"):
        r["roofline"]["frac_source"] = "profiles/r06_bench_kernel_stats.csv: 11 symbols, 34.0 launches and 0.765 ms per step over 15 traced steps"
    return r


@pytest.mark.parametrize("path", _full_records())
def test_line_fits_the_driver_tail_with_both_halves(path):
    rec = json.load(open(path))
    for r in (rec, _worst_case(rec)):
        line = bench.compact_record(r, "gpurun_out/bench_full.json")
        assert len(line) <= bench.LINE_LIMIT <= 6144, len(line)
        assert "\n" not in line
        out = json.loads(line)
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert k in out, k
        for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert k in out["roofline"], k
        h = out["hifi_gan"]                      # the metric's second half, inside the last 8 KB whatever follows it
        assert h["rtf"] > 0 and h["ms_per_batch"] > 0 and "mfma_roofline_frac" in h and "cpu_baseline" in h
        assert line.rfind('"hifi_gan"') > len(line) - 8192
        assert abs(out["value"] - r["value"]) <= 1e-5 * r["value"] and abs(out["ms_per_step"] - r["ms_per_step"]) <= 1e-5 * r["ms_per_step"]


def test_plain_run_does_only_the_headline_legs():
    """bench.plan_legs: a plain run times the HiFi-GAN batch beside the step and nothing else; --full adds every other leg and the long
    record, each --no-* option leaving its leg out; on more than one GPU a --full run adds the roofline alone."""
    base = ["--gpus", "1", "--steps", "5", "--warmup", "2"]
    assert bench.parse_args(base).full is False
    on = lambda argv, world=1: sorted(k for k, v in bench.plan_legs(bench.parse_args(argv), world).items() if v)
    everything = ["cpu_baseline", "e2e", "extra", "full_record", "hifi_gan", "hifi_stages", "mel", "roofline"]
    assert on(base) == ["hifi_gan"]
    assert on(base + ["--dump-outputs", "d"]) == ["hifi_gan"]
    assert on(base + ["--no-hifi"]) == []
    assert on(base + ["--full"]) == everything
    assert on(base + ["--full", "--no-roofline", "--no-cpu-baseline", "--no-hifi"]) == ["e2e", "extra", "full_record", "mel"]
    assert on(base + ["--full", "--no-extra", "--no-e2e", "--no-mel"]) == ["cpu_baseline", "full_record", "hifi_gan", "hifi_stages", "roofline"]
    assert on(["--gpus", "2", "--full"], 2) == ["full_record", "roofline"]
    assert on(["--gpus", "2"], 2) == []


def test_plain_record_compacts_to_a_complete_line():
    """compact_record on what a plain run records (no roofline, CPU baselines, HiFi-GAN stages or auxiliary legs, no side file): the
    line still carries every contract key and both halves of the metric."""
    rec = json.load(open(_full_records()[-1]))
    plain = {k: rec[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                 "vs_baseline", "dtype", "data", "config", "mel_frames_per_s_per_gpu", "model_tflops",
                                 "step_mfma_roofline_frac", "final_losses", "hifi_gan")}
    plain["hifi_gan"] = {k: v for k, v in plain["hifi_gan"].items() if k not in ("stages", "cpu_baseline")}
    out = json.loads(bench.compact_record(plain))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "final_losses"):
        assert k in out, k
    for k in ("roofline", "cpu_baseline", "aux", "full_record"):
        assert k not in out, k
    assert out["hifi_gan"]["rtf"] > 0 and "stages" not in out["hifi_gan"]
    assert out["metric"] == rec["metric"] and out["unit"] == rec["unit"] and out["dtype"] == rec["dtype"]
    assert abs(out["value"] - rec["value"]) <= 1e-5 * rec["value"] and abs(out["ms_per_step"] - rec["ms_per_step"]) <= 1e-5 * rec["ms_per_step"]


def test_line_refuses_to_grow_silently():
    rec = json.load(open(_full_records()[-1]))
    rec["config"]["workload"] = "x" * 7000
    with pytest.raises(RuntimeError):
        bench.compact_record(rec)


def test_roofline_frac_follows_from_the_committed_rocprof_summary():
    """family GF per step / (sum of the family's TotalDurationNs / traced steps) from profiles/r*_bench_kernel_stats.csv, recomputed here by hand."""
    import csv
    prof = bench.profile_family_time("win_conv_kernel")
    assert prof is not None
    rows = list(csv.DictReader(open(os.path.join(ROOT, prof["source"]))))
    steps = sum(int(r["Calls"]) for r in rows if "adam_pack_kernel" in r["Name"] or "adam_clip_kernel" in r["Name"])
    ns = sum(float(r["TotalDurationNs"]) for r in rows if "win_conv_kernel" in r["Name"])
    assert steps == prof["steps_traced"] and abs(prof["ms_per_step"] - ns / steps * 1e-6) < 1e-9
    tag = os.path.basename(prof["source"]).split("_bench_kernel_stats")[0]
    full = os.path.join(ROOT, "profiles", tag + "_bench.json")
    if os.path.exists(full):
        r = json.load(open(full))["roofline"]
        if r.get("family") == "win_conv" and "frac_source" in r and r["frac_source"].startswith("profiles/"):
            gf = [f for f in r["families"] if f["family"] == "win_conv"][0]["gflop"]
            assert abs(r["frac"] - gf / prof["ms_per_step"] / 2500.0) <= 0.03 * r["frac"]


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    """--dump-outputs: float32 / float64 .npy per array; an array over its share of the limit becomes a fixed sample of its flattened
    elements with the sampled indices beside it, the same on every run."""
    import numpy as np
    import torch
    mel = torch.arange(16 * 423 * 80, dtype=torch.float32).view(16, 423, 80).to(torch.bfloat16)
    lens = torch.tensor([423, 400], dtype=torch.int64)
    masks = torch.zeros(2, 5, dtype=torch.bool)
    fwd = (mel, None, None, None, None, masks, None, lens, None)
    arrays = bench.step_arrays((torch.ones(6), fwd))
    assert set(arrays) == {"losses", "mel", "src_masks", "mel_lens"}
    assert arrays["mel"].dtype == np.float32 and arrays["mel_lens"].dtype == np.float64 and arrays["src_masks"].dtype == np.float64
    limit = 1 << 20
    for d in ("a", "b"):
        bench.dump_outputs(arrays, str(tmp_path / d), limit=limit)
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert total <= limit, total
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == ["losses.npy", "mel.index.npy", "mel.npy", "mel_lens.npy", "src_masks.npy"]
    idx = np.load(tmp_path / "a" / "mel.index.npy")
    sample = np.load(tmp_path / "a" / "mel.npy")
    assert np.array_equal(sample, arrays["mel"].reshape(-1)[idx]) and np.all(np.diff(idx) > 0)
    for f in (tmp_path / "a").iterdir():
        assert np.array_equal(np.load(f), np.load(tmp_path / "b" / f.name))
    assert np.array_equal(np.load(tmp_path / "a" / "mel_lens.npy"), [423.0, 400.0])
