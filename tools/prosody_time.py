"""Time the per-phoneme prosody route of batched text -> mel against the existing `generate_mel([...])` route on one MI355X.

For the README's workloads (seeded: 8 and 32 texts of 20-120 phonemes, per-utterance speakers), with every graph captured, alternating
in one process, every timed call between two device synchronisations:

  existing     `generate_mel(texts)` with scalar controls -- the route of DESIGN.md section 12, the baseline
  neutral      the new route with neutral inputs (all-ones per-phoneme controls): the same mels on the per-row kernels + the fit launch
  controls     per-phoneme pitch / energy / duration controls
  budget       per-phoneme controls and a frame budget (`target_frames`) per text

and each variant's median over the existing route's.  The host-side normalisation of the arrays is inside the timed call.

    python tools/prosody_time.py --out profiles/prosody_time.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.batch_synth_time import make_tts, texts_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prosody_time.json"))
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    import numpy as np
    import torch
    from tts_king_amd import lib
    tts = make_tts(True)
    fs = tts.tts._synth
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "reps": args.reps,
              "unit": "ms per call over all texts, host clock between two device synchronisations", "workloads": {}}
    rnd = random.Random(1234)
    for n in (8, 32):
        texts = texts_of(rnd, n)
        spk = [rnd.randint(0, 65) for _ in range(n)]
        rng = np.random.RandomState(n)
        ones = [np.ones(len(t), np.float32) for t in texts]
        ctl = [[(rng.rand(len(t)) * 0.6 + 0.7).astype(np.float32) for t in texts] for _ in range(3)]
        natural = [int(x.shape[1]) for x in tts.generate_mel(texts, speaker=spk)]
        hi = max(natural)                       # budgets within the longest natural length: the same frame bucket as the other variants
        targets = [min(max(int(t * f), 1), hi) for t, f in zip(natural, rng.rand(n) * 0.6 + 0.7)]
        variants = {
            "existing": lambda: tts.generate_mel(texts, speaker=spk),
            "neutral": lambda: tts.generate_mel(texts, ones, ones, ones, speaker=spk),
            "controls": lambda: tts.generate_mel(texts, ctl[0], ctl[1], ctl[2], speaker=spk),
            "budget": lambda: tts.generate_mel(texts, ctl[0], ctl[1], ctl[2], speaker=spk, target_frames=targets),
        }
        for c in (fs._front, fs._back):          # one workload's graphs at a time
            c.clear()
        for fn in variants.values():             # first sight eager, second captured, third replayed
            for _ in range(3):
                fn()
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0))
        a, b = variants["existing"](), variants["neutral"]()
        row = {"phonemes": [len(t) for t in texts], "frames": natural, "target_frames": targets,
               "neutral_equals_existing": all(torch.equal(x, y) for x, y in zip(a, b)),
               "budget_met": [int(x.shape[1]) for x in variants["budget"]()] == targets,
               "graphs_held": {"front": [list(k) for k in fs._front], "back": len(fs._back)}}
        for k, v in times.items():
            row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}
        for k in ("neutral", "controls", "budget"):
            row[k + "_over_existing"] = round(row[k]["median_ms"] / row["existing"]["median_ms"], 3)
        result["workloads"]["%d_texts_20_120" % n] = row
        print(n, json.dumps({k: v for k, v in row.items() if k.endswith("_over_existing") or k in ("neutral_equals_existing", "budget_met")}),
              json.dumps({k: v["median_ms"] for k, v in row.items() if isinstance(v, dict) and "median_ms" in v}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
