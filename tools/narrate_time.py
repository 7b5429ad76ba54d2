"""Time a paragraph in one call (`TTSKing.narrate`) against the per-sentence route joined on the host, on one MI355X.

Workload: 40 sentences in the order given, 32 of 150-900 frames and 8 of 17-95 (random phoneme ids on the seeded random-init models,
the frame counts set through per-sentence duration controls; the counts actually reached are in the file).

    python tools/narrate_time.py --out profiles/narrate_time.json

Route A is `narrate(texts, ...)`: per group of 32 one `mel_ragged` call, one vocoder graph that ends in the two join launches, one
copy of the joined int16 waveform to the host.  Route B is `speak(texts, ...)` (the same batched text-to-mel and vocoder), then
every sentence's float waveform copied to the host and joined there by the numpy restatement of the join (tests/join_ref.py) --
what a caller does without `narrate`.  Both run in one process, alternated, every graph captured before the first timed call, host
clock around the whole call; medians and minima in ms.  Also the two join launches' device time alone (HIP events around 20
back-to-back launches on the first group's flat buffer) and the bytes each route copies to the host.
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


def workload(tts):
    """(texts, duration controls, frames reached): 32 sentences aimed at 150 .. 900 frames and 8 at 17 .. 95, interleaved."""
    import numpy as np
    rnd = random.Random(11)
    aims = [175 + (700 * i) // 31 for i in range(32)]          # inside 150 .. 900 by the rounding of the controls
    rnd.shuffle(aims)
    short = [27 + (56 * i) // 7 for i in range(8)]           # inside 17 .. 95 likewise
    for k, t in enumerate(short):
        aims.insert(5 * k + 2, t)
    texts = [np.array([rnd.randint(1, 206) for _ in range(max(6, min(120, t // 4)))], dtype=np.int64) for t in aims]
    base = [int(m.shape[1]) for m in tts.generate_mel(texts)]
    dc = [max(0.25, round(4.0 * t / max(b, 1)) / 4.0) for t, b in zip(aims, base)]      # quarters: whole frames per phoneme stay whole
    frames = [int(m.shape[1]) for m in tts.generate_mel(texts, dc)]
    return texts, dc, frames


def host_join(wavs, join, rate):
    """Route B's second half: the sentences' float waveforms, on the host, through the restatement -> int16."""
    import numpy as np
    from tests import join_ref
    from tts_king_amd import narrate
    lens = [w.size for w in wavs]
    table = join.table(np.cumsum([0] + lens[:-1]).tolist(), lens)
    return join_ref.join_ref(np.concatenate(wavs), table, narrate.out_bound(table), 32768.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "narrate_time.json"))
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    import numpy as np
    import torch
    from tools.batch_synth_time import make_tts
    from tts_king_amd import lib, narrate, ops
    tts = make_tts(True)
    texts, dc, frames = workload(tts)
    rate = tts.vocoder.output_rate(None)
    join = narrate.Join(narrate.settings(rate), narrate.pause_plan([""] * len(texts), rate))
    groups = narrate.groups(len(texts))

    def route_a():
        return tts.narrate(texts, duration_control=dc)

    def route_b():
        parts = []
        for lo, hi in groups:
            wavs = tts.speak(texts[lo:hi], dc[lo:hi])
            host = [w.cpu().numpy().reshape(-1) for w in wavs]                # what a caller does: N copies
            r = host_join(host, join.part(lo, hi), rate)
            parts.append(r["out"][:r["total"]])
        return np.concatenate(parts).reshape(1, 1, -1)

    for fn in (route_a, route_b):                        # first sight eager, second captured, third replayed
        for _ in range(3):
            out = fn()
    a, b = route_a(), route_b()
    times = {"narrate": [], "speak_then_host_join": []}
    for _ in range(args.reps):
        for k, fn in (("narrate", route_a), ("speak_then_host_join", route_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(1e3 * (time.perf_counter() - t0))
    # the host half of route B alone, and the join launches alone
    wavs = [w.cpu().numpy().reshape(-1) for w in tts.speak(texts[:32], dc[:32])]
    host_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        host_join(wavs, join.part(0, 32), rate)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    mels = tts.generate_mel(texts[:32], dc[:32])
    gen = tts.vocoder.model
    flat, plan, spf = gen.forward_ragged_flat(mels, True)
    offs, lens = gen.join_spans(plan, spf, flat.numel(), {})
    table = join.part(0, 32).table(offs, lens, rows=plan.N)
    tab = torch.from_numpy(table).to(flat.device)
    out = torch.empty(narrate.out_bound(table), dtype=torch.int16, device=flat.device)
    info = torch.empty(plan.N + 1, narrate.ROW, dtype=torch.int32, device=flat.device)
    ops.wav_join(flat, tab, out=out, info=info, int16_scale=32768.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ops.wav_join(flat, tab, out=out, info=info, int16_scale=32768.0)
    e1.record()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "reps": args.reps, "rate": rate,
              "unit": "ms per call of the whole paragraph, host clock, graphs replayed, device-to-host copies included",
              "sentences": len(texts), "groups": len(groups), "frames": frames, "frames_total": sum(frames),
              "long_in_150_900": sum(150 <= f <= 900 for f in frames), "short_in_17_95": sum(17 <= f <= 95 for f in frames),
              "samples_out": int(a.shape[-1]), "same_length": bool(a.shape == b.shape),
              "max_abs_difference_int16": int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) if a.shape == b.shape else None,
              "graphs": {"front": len(tts.tts._synth._front), "back": len(tts.tts._synth._back), "vocoder": len(tts.vocoder._synth._rag)},
              "narrate": {"median_ms": round(med["narrate"], 3), "min_ms": round(min(times["narrate"]), 3), "d2h_copies": 2 * len(groups)},
              "speak_then_host_join": {"median_ms": round(med["speak_then_host_join"], 3), "min_ms": round(min(times["speak_then_host_join"]), 3),
                                       "d2h_copies": len(texts), "d2h_bytes": int(sum(f * spf * 4 for f in frames)),
                                       "host_join_of_32_alone_median_ms": round(statistics.median(host_ms), 3)},
              "narrate_over_host_route": round(med["narrate"] / med["speak_then_host_join"], 4),
              "join_launches_device_us": {"rows": int(plan.N), "source_samples": int(flat.numel()), "dst_samples": int(out.numel()),
                                          "both_launches": round(1e3 * e0.elapsed_time(e1) / 20, 2)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("narrate", "speak_then_host_join", "narrate_over_host_route", "join_launches_device_us", "graphs",
                                             "long_in_150_900", "short_in_17_95", "max_abs_difference_int16")}))


if __name__ == "__main__":
    main()
