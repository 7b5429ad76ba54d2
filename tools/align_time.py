"""Time forced alignment on one MI355X.

32 pairs of 150-900 frames (the lengths of tools/window_vocoder_time.py), C = 80:

    python tools/align_time.py --out profiles/align_time.json

* `ops.dtw_align` on all 32 pairs as ONE launch (Gaussian features, y a random warp of x plus noise, both of the pair's length):
  device time between two HIP events after warm-up, median over repeats; the two kernels' shares of it from one pass under
  torch.profiler (their summed device durations), "not measured" when the profiler reports no kernels.
* `TTSKing.align` on 32 synthetic recordings of the same frame counts (random-init model, one phoneme per about 8 frames): wall
  time of the 32 calls one after the other, and of one list call of all 32 (`Aligner.align`), each ended by a device synchronise.
* tests/dtw_ref.py (fp64 numpy, vectorised by anti-diagonal) over the same 32 pairs in one process of this host, for scale.
No time is fixed here: there is no counterpart on an earlier commit."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HOP, C = 256, 80
PHONES = ["R", "A", "B", "O0", "T", "A"]


def pairs(lens):
    import numpy as np
    from tests import dtw_ref
    out = []
    for T in lens:
        rng = np.random.default_rng(T)
        Tx = T - T // 5
        x = rng.standard_normal((Tx, C)).astype(np.float32)
        y = (x[dtw_ref.make_warp(rng, Tx, T)] + 0.3 * rng.standard_normal((T, C))).astype(np.float32)
        out.append((x, y))
    return out


def kernel_shares(fn):
    """Summed device durations of the two kernels over one call of fn, from torch.profiler; None when it reports neither."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        tot = {"dtw_cost_kernel": 0.0, "dtw_path_kernel": 0.0}
        for ev in prof.events():
            for k in tot:
                if k in ev.name:
                    tot[k] += float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
    except Exception as e:                        # a profiler that cannot start is a missing figure, not a failed run
        return None, "torch.profiler: %s" % e
    if not any(tot.values()):
        return None, "torch.profiler reported no dtw kernels"
    return {k: round(v / 1e3, 4) for k, v in tot.items()}, "ms, summed device durations from torch.profiler over one launch"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_time.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
    args = ap.parse_args()
    import numpy as np
    import torch
    from tests import dtw_ref, pitch_ref
    from tools.window_vocoder_time import workloads
    from tts_king_amd import lib, ops
    lens = workloads()["32_utterances_150_900"]
    prs = pairs(lens)
    dev = "cuda:0"
    B, ldx, ldy = len(prs), max(p[0].shape[0] for p in prs), max(p[1].shape[0] for p in prs)
    x = torch.zeros(B, ldx, C, device=dev)
    y = torch.zeros(B, ldy, C, device=dev)
    for b, (xb, yb) in enumerate(prs):
        x[b, :len(xb)], y[b, :len(yb)] = torch.from_numpy(xb), torch.from_numpy(yb)
    xl = torch.tensor([len(p[0]) for p in prs], dtype=torch.int32, device=dev)
    yl = torch.tensor([len(p[1]) for p in prs], dtype=torch.int32, device=dev)
    seg = torch.zeros(B, 128, dtype=torch.int32, device=dev)
    ns = []
    for b, (xb, _) in enumerate(prs):
        n = max(len(xb) // 8, 1)
        d = np.full(n, len(xb) // n, dtype=np.int32)
        d[-1] += len(xb) - int(d.sum())
        seg[b, :n] = torch.from_numpy(d)
        ns.append(n)
    ns = torch.tensor(ns, dtype=torch.int32, device=dev)
    launch = lambda: ops.dtw_align(x, y, xl, yl, seg, ns)
    for _ in range(3):
        out = launch()
    torch.cuda.synchronize()
    assert out[2].cpu().tolist() == [0] * B
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    shares, how = kernel_shares(launch)
    cells = int(sum(len(a) * len(b) for a, b in prs))
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "reps": args.reps, "pairs": B, "channels": C,
              "lens_frames": lens, "cells": cells, "workspace_bytes": int(lib.load().ttsk_dtw_workspace_bytes(B, ldx, ldy)),
              "dtw_align_one_launch_of_32": {"unit": "ms of device time between two HIP events (includes the workspace allocation's host time "
                                                     "only as far as it delays the enqueue), median over repeats",
                                             "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4),
                                             "max_ms": round(max(times), 4)},
              "kernels": shares if shares is not None else "not measured", "kernels_unit": how}
    # TTSKing.align on recordings of the same frame counts
    import tts_king
    tts = tts_king.TTSKing(os.path.join(ROOT, "config.yaml"))
    wavs = [pitch_ref.glide(HOP * (T - 1) + 17, np.random.default_rng(T), f_lo=100.0 + T % 90, noise=(T // 3, T // 3 + 12), silent=None) for T in lens]
    texts = [tts.text_preprocess("{" + " ".join(PHONES[i % 6] for i in range(max(T // 8, 1))) + "}") for T in lens]
    for w, t in zip(wavs, texts):                  # warm-up: every shape once
        tts.align(w, t)
    tts._aligner.align(wavs, texts, tts.speakers[0], 22050)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solo = [tts.align(w, t) for w, t in zip(wavs, texts)]
    torch.cuda.synchronize()
    t_solo = time.perf_counter() - t0
    t0 = time.perf_counter()
    both = tts._aligner.align(wavs, texts, tts.speakers[0], 22050)
    torch.cuda.synchronize()
    t_list = time.perf_counter() - t0
    result["tts_king_align"] = {"unit": "s of wall time, ended by a device synchronise, after one warm-up pass", "frames": [r["frames"] for r in solo],
                                "32_calls_s": round(t_solo, 4), "one_list_call_of_32_s": round(t_list, 4),
                                "list_equals_solo": all(a["durations"].tolist() == b["durations"].tolist() for a, b in zip(solo, both)),
                                "mean_cost_per_frame": round(float(np.mean([r["cost_per_frame"] for r in solo])), 4)}
    if not args.no_host:
        t0 = time.perf_counter()
        same = 0
        px = out[0].cpu().numpy()
        for b, (xb, yb) in enumerate(prs):
            same += int(dtw_ref.dtw(xb, yb)[2].tolist() == px[b, :len(yb)].tolist())
        result["host"] = {"what": "tests/dtw_ref.py in fp64 numpy over the same 32 pairs, one process of this host", "s": round(time.perf_counter() - t0, 3),
                          "pairs_with_the_kernel's_path": same}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
