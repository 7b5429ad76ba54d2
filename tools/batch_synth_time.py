"""Time batched text -> mel (`TTSKing.generate_mel([...])`, `speak([...])`) against the per-utterance loop on one MI355X, and count graphs.

For seeded workloads (8 and 32 texts of 20-120 phonemes, per-utterance speakers), alternating in one process, warm, every timed call
between two device synchronisations:

  mel_loop     a loop of `generate_mel(text)` with every text's graphs already captured (the per-utterance path's best case: a
               caller that repeats texts) -- the baseline
  mel_batch    one `generate_mel([texts])`
  speak_loop   a loop of `speak(text)`, graphs captured
  speak_batch  one `speak([texts])`

then the number of graphs each route holds (and of distinct keys it met) after 200 random texts.

    python tools/batch_synth_time.py --out profiles/batch_synth_time.json

`--launches existing|batched --calls N` instead runs N plain (uncaptured) calls of one route's two halves at the padded shape B = 4,
L = 48, T = 256 and exits: under `rocprofv3 --kernel-trace --stats` the difference of two call counts gives the launches per call
(profiles/batch_synth_kernel_counts.txt).
"""
import argparse
import copy
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_tts(hip_graph=True):
    import torch
    import yaml
    import tts_king
    from tts_king_amd.config import default_config
    cfg = copy.deepcopy(default_config())
    cfg.mi355x["hip_graph"] = hip_graph
    with tempfile.NamedTemporaryFile("w", suffix=".yaml", delete=False) as f:
        yaml.safe_dump(json.loads(json.dumps(cfg)), f)
    try:
        t = tts_king.TTSKing(f.name)
    finally:
        os.unlink(f.name)
    with torch.no_grad():       # random-init duration head predicts ~0 frames: a few frames per phoneme, as a trained model gives
        t.tts.model.get("variance_adaptor.duration_predictor.linear_layer.bias").fill_(1.3)
    return t


def texts_of(rnd, n, lo=20, hi=120):
    import numpy as np
    return [np.array([rnd.randint(1, 206) for _ in range(rnd.randint(lo, hi))], dtype=np.int64) for _ in range(n)]


def launches(route, calls):
    import torch
    tts = make_tts(False)
    m = tts.tts.model
    m.eval()
    dev = m.device
    g = torch.Generator().manual_seed(5)
    lens = (48, 31, 17, 40)
    ids = torch.zeros(4, 48, dtype=torch.int64)
    for u, L in enumerate(lens):
        ids[u, :L] = torch.randint(1, 207, (L,), generator=g)
    ids, spk = ids.to(dev), torch.tensor([5, 9, 2, 30], device=dev)
    ones = torch.ones(4, device=dev)
    with torch.no_grad():
        for _ in range(calls):
            if route == "batched":
                x3, dur, total, _ = m.eval_front_ragged(spk, ids, torch.tensor(lens, device=dev), 48, ones, ones, ones)
                total.cpu()
                m.eval_back_ragged(x3, dur, 48, 256)
            else:
                x3, dur, total, _ = m.eval_front(spk, ids, torch.full((4,), 48, dtype=torch.int64, device=dev), 48)
                total.cpu()
                m.eval_back(x3, dur, 48, 256)
    torch.cuda.synchronize()
    print("%s: %d calls done" % (route, calls))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_synth_time.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--launches", choices=("existing", "batched"))
    ap.add_argument("--calls", type=int, default=2)
    args = ap.parse_args()
    if args.launches:
        return launches(args.launches, args.calls)
    import torch
    from tts_king_amd import lib
    tts = make_tts(True)
    fs, voc = tts.tts._synth, tts.vocoder._synth
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "reps": args.reps,
              "unit": "ms per call over all texts, host clock between two device synchronisations", "workloads": {}}
    rnd = random.Random(1234)
    for n in (8, 32):
        texts = texts_of(rnd, n)
        spk = [rnd.randint(0, 65) for _ in range(n)]
        singles = [t[None] for t in texts]
        variants = {
            "mel_loop": lambda: [tts.generate_mel(t, speaker=s) for t, s in zip(singles, spk)],
            "mel_batch": lambda: tts.generate_mel(texts, speaker=spk),
            "speak_loop": lambda: [tts.speak(t, speaker=s) for t, s in zip(singles, spk)],
            "speak_batch": lambda: tts.speak(texts, speaker=spk),
        }
        for c in (fs._front, fs._back, voc._voc, voc._rag):       # one workload's graphs at a time
            c.clear()
        for fn in variants.values():                               # first sight eager, second captured, third replayed
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
        mels = tts.generate_mel(texts, speaker=spk)
        row = {"phonemes": [len(t) for t in texts], "frames": [int(x.shape[1]) for x in mels]}
        for k, v in times.items():
            row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}
        row["mel_loop_over_batch"] = round(row["mel_loop"]["median_ms"] / row["mel_batch"]["median_ms"], 3)
        row["speak_loop_over_batch"] = round(row["speak_loop"]["median_ms"] / row["speak_batch"]["median_ms"], 3)
        result["workloads"]["%d_texts_20_120" % n] = row
        print(n, json.dumps({k: v["median_ms"] for k, v in row.items() if isinstance(v, dict)}), flush=True)
    # graphs after 200 random texts: the loop meets a new key for almost every text, the batched route a few buckets
    rnd = random.Random(99)
    texts = texts_of(rnd, 200)
    counts = {}
    for route in ("loop", "batch"):
        for c in (fs._front, fs._back):
            c.clear()
        fs._seen.clear()
        for _ in range(2):                                         # a key is captured at its second sight
            if route == "loop":
                for t in texts:
                    tts.generate_mel(t[None])
            else:
                for i in range(0, 200, 8):
                    tts.generate_mel(texts[i:i + 8])
        counts[route] = {"graphs_held": len(fs._front) + len(fs._back), "front_keys_met": len([k for k in fs._seen if k[0] == "front"]),
                         "back_keys_met": len([k for k in fs._seen if k[0] == "back"]), "max_graphs_per_cache": fs.max_graphs}
    result["graphs_after_200_texts"] = counts
    print(json.dumps(counts))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
