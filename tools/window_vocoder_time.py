"""Time windowed vocoding against the per-utterance paths on one MI355X, and sweep the window size.

For seeded workloads a user would run (8 utterances of 150-900 frames; one utterance of 1000 frames; 32 utterances), alternating in
one process, warm, every call ending in its device-to-host copy (so the device is idle when the clock stops):

  ragged[W]   HIFIapi.generate_ragged (graph replayed) with tts_king_amd.windows.W set to each candidate
  graph_loop  a loop of HIFIapi.generate over the same utterances, every length's graph already captured (the per-utterance
              path's best case: a caller that repeats lengths)
  eager_loop  the same loop on plain launches (its usual case: a length seen for the first time)

    python tools/window_vocoder_time.py --out profiles/window_vocoder_time.json

Writes medians and minima in ms, the ratios graph_loop / ragged and eager_loop / ragged (> 1: windows are faster), and the window
size with the smallest summed median over the workloads.  tts_king_amd.windows.W is a constant: this tool is where it is chosen.
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

CANDIDATES = (64, 96, 128, 192, 256)


def workloads(seed=1234):
    rnd = random.Random(seed)
    return {"8_utterances_150_900": [rnd.randint(150, 900) for _ in range(8)],
            "1_utterance_1000": [1000],
            "32_utterances_150_900": [rnd.randint(150, 900) for _ in range(32)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_vocoder_time.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--windows", default=",".join(str(w) for w in CANDIDATES))
    args = ap.parse_args()
    import torch
    from hifiapi import HIFIapi
    from tts_king_amd import lib, windows
    from tts_king_amd.config import default_config
    from tts_king_amd.synthetic import make_mel
    cands = [int(w) for w in args.windows.split(",")]
    shipped = windows.W

    def api(graph):
        c = copy.deepcopy(default_config())
        c.model_config["vocoder"]["use_cpu"] = False
        c.mi355x["hip_graph"] = graph
        return HIFIapi(c, "cuda:0")

    graphed, eager = api(True), api(False)
    H = graphed.model.halo()
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "halo_frames": H, "reps": args.reps,
              "candidates": cands, "unit": "ms per call, host clock around the call (device-to-host copy included)", "workloads": {}}
    for name, lens in workloads().items():
        mels = [make_mel(1, T, seed=T)[0].to("cuda:0") for T in lens]
        batches = [m.unsqueeze(0) for m in mels]

        def ragged(w):
            windows.W = w
            return graphed.generate_ragged(mels)

        variants = {"ragged_W%d" % w: (lambda w=w: ragged(w)) for w in cands}
        variants["graph_loop"] = lambda: [graphed.generate(b) for b in batches]
        variants["eager_loop"] = lambda: [eager.generate(b) for b in batches]
        graphed._synth._voc.clear()                      # the per-length cache holds 32 graphs: one workload's lengths at a time
        for fn in variants.values():                     # first sight eager, second captured, third replayed
            for _ in range(3):
                fn()
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append(1e3 * (time.perf_counter() - t0))
        row = {"lens": lens, "frames": sum(lens)}
        for k, v in times.items():
            row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}
        for w in cands:
            p = windows.plan_windows(lens, w, H)
            r = row["ragged_W%d" % w]
            r.update(N=p.N, windows=p.n_windows, solo_utterances=len(p.short), window_frames=p.N * w,
                     graph_loop_over_ragged=round(row["graph_loop"]["median_ms"] / r["median_ms"], 3),
                     eager_loop_over_ragged=round(row["eager_loop"]["median_ms"] / r["median_ms"], 3))
        result["workloads"][name] = row
        print(name, json.dumps({k: v["median_ms"] for k, v in row.items() if isinstance(v, dict)}), flush=True)
    windows.W = shipped
    total = {w: round(sum(r["ragged_W%d" % w]["median_ms"] for r in result["workloads"].values()), 4) for w in cands}
    result["summed_median_ms"] = {str(w): t for w, t in total.items()}
    result["fastest_window"] = min(total, key=total.get)
    result["shipped_window"] = shipped
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"summed_median_ms": result["summed_median_ms"], "fastest_window": result["fastest_window"], "shipped_window": shipped}))


if __name__ == "__main__":
    main()
