"""Time short utterances as rows of the windowed batch against the routes they took before, on one MI355X.

For seeded workloads a service answering with short phrases would run (8 and 32 utterances of 17-95 frames; 8 utterances mixed
17-400; one utterance of 50 frames), alternating in one process, warm, every call ending in its device-to-host copy (so the device
is idle when the clock stops):

  rows          HIFIapi.generate_ragged (graph replayed): every utterance of at least one frame a row of the (N, W, 80) batch
  solo_ragged   the same call on a generator whose `short_rows()` answers False: the windowed batch for the utterances that fill a
                window, `GraphedSynthesizer.wav` (one captured graph per length) for each shorter one — the list call as it was
  graph_loop    a loop of HIFIapi.generate over the utterances, every length's graph already captured
  eager_loop    the same loop on plain launches (a length seen for the first time)

    python tools/short_vocoder_time.py --out profiles/short_vocoder_time.json
    rocprofv3 --kernel-trace --stats ... -- python tools/short_vocoder_time.py --launches 10      (the launch list of the route)

Writes medians and minima in ms, the ratios of each earlier route over `rows` (> 1: rows are faster), the plan of each workload and
the largest int16 difference between `rows` and `graph_loop` on the same mels (the two routes pick different kernels for a V1
generator; tests/test_short_rows_gpu.py holds the bars).  `--launches N`: nothing is timed; the 8-utterance short workload runs N
times on plain launches (`Generator.forward_ragged`, after the weights are packed by one `forward`), so that a kernel trace of the
process divides by N into the launches of one call (profiles/short_vocoder_kernel_counts.txt).
"""
import argparse
import copy
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def workloads(seed=1234):
    rnd = random.Random(seed)
    return {"8_utterances_17_95": [rnd.randint(17, 95) for _ in range(8)],
            "32_utterances_17_95": [rnd.randint(17, 95) for _ in range(32)],
            "8_utterances_17_400": [rnd.randint(17, 400) for _ in range(8)],
            "1_utterance_50": [50]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "short_vocoder_time.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--launches", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from hifiapi import HIFIapi
    from tts_king_amd import lib, windows
    from tts_king_amd.config import default_config
    from tts_king_amd.synthetic import make_mel

    def api(graph):
        c = copy.deepcopy(default_config())
        c.model_config["vocoder"]["use_cpu"] = False
        c.mi355x["hip_graph"] = graph
        return HIFIapi(c, "cuda:0")

    if args.launches:
        gen = api(False).model
        mels = [make_mel(1, T, seed=T)[0].to("cuda:0") for T in workloads()["8_utterances_17_95"]]
        gen(mels[0].unsqueeze(0))
        for _ in range(args.launches):
            gen.forward_ragged(mels)
        torch.cuda.synchronize()
        return
    graphed, solo, eager = api(True), api(True), api(False)
    solo.model.short_rows = lambda: False                # the list call as it was: short utterances one by one
    assert graphed.model.short_rows()
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "window_frames": windows.W, "reps": args.reps,
              "unit": "ms per call, host clock around the call (device-to-host copy included)", "workloads": {}}
    for name, lens in workloads().items():
        mels = [make_mel(1, T, seed=T)[0].to("cuda:0") for T in lens]
        batches = [m.unsqueeze(0) for m in mels]
        variants = {"rows": lambda: graphed.generate_ragged(mels),
                    "solo_ragged": lambda: solo.generate_ragged(mels),
                    "graph_loop": lambda: [graphed.generate(b) for b in batches],
                    "eager_loop": lambda: [eager.generate(b) for b in batches]}
        graphed._synth._voc.clear()                      # the per-length caches: one workload's lengths at a time
        solo._synth._voc.clear()
        outs = {}
        for k, fn in variants.items():                   # first sight eager, second captured, third replayed
            for _ in range(3):
                outs[k] = fn()
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append(1e3 * (time.perf_counter() - t0))
        plan, old = graphed.model.plan(lens), solo.model.plan(lens)
        row = {"lens": lens, "frames": sum(lens), "N": plan.N, "rows": None, "rows_in_batch": plan.n_windows, "batch_frames": plan.N * windows.W,
               "solo_ragged_N": old.N, "solo_ragged_solo_utterances": len(old.short),
               "vocoder_graphs": {"rows": len(graphed._synth._rag), "solo_ragged": len(solo._synth._rag) + len(solo._synth._voc),
                                  "graph_loop": len(graphed._synth._voc)},
               "max_int16_difference_rows_vs_graph_loop": max(int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())
                                                              for a, b in zip(outs["rows"], outs["graph_loop"]))}
        for k, v in times.items():
            row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}
        for k in ("solo_ragged", "graph_loop", "eager_loop"):
            row["rows"][k + "_over_rows"] = round(row[k]["median_ms"] / row["rows"]["median_ms"], 3)
        result["workloads"][name] = row
        print(name, json.dumps({k: v["median_ms"] for k, v in row.items() if isinstance(v, dict) and "median_ms" in v}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
