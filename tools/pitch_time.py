"""Time the data-preparation kernels on one MI355X against their fp64 restatement on the host.

32 synthetic utterances of 150-900 frames (the lengths of tools/window_vocoder_time.py), one utterance per call as
tts_king_amd/preprocess.py runs them, every call warmed, no graph:

    python tools/pitch_time.py --out profiles/pitch_time.json

Per stage -- `PitchExtractor` (ttsk_pitch_yin), `TacotronSTFT` (ttsk_stft_frames + ttsk_gemm + ttsk_mel_from_spec) and the phoneme-level
reduction (ttsk_phoneme_prosody) -- the device time of the 32 calls between two HIP events, as the median over repeats in which the
stages alternate.  Also ttsk_pitch_yin on all 32 rows as one ragged launch, and from its time the rates the kernel reaches: the
(sample, lag) pairs per second against the vector peak and the LDS bytes it reads per second.  The baseline is tests/pitch_ref.py
(fp64 numpy, vectorised over lags) over the same arrays on up to 16 processes of this host, measured before the GPU is opened."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HOP = 256


def signals():
    import numpy as np
    from tests import pitch_ref
    from tools.window_vocoder_time import workloads
    lens = workloads()["32_utterances_150_900"]
    return lens, [pitch_ref.glide(HOP * T, np.random.default_rng(T), f_lo=100.0 + T % 90, noise=(T // 3, T // 3 + 12), silent=(T // 2, T // 2 + 8))
                  for T in lens]


def _yin64(y):
    from tests import pitch_ref
    return pitch_ref.yin(y)[0]


def host_baseline(wavs, procs):
    import multiprocessing as mp
    t0 = time.perf_counter()
    with mp.get_context("fork").Pool(procs) as pool:
        f0 = pool.map(_yin64, wavs, chunksize=1)
    return time.perf_counter() - t0, f0


def accuracy(pe, dev):
    """The composite case of tests/test_pitch_gpu.py, measured here so that the figures travel with the timings: the share of frames
    whose decision margin is under 1e-4 (left out), and on the others the largest relative f0 deviation from the fp64 restatement of
    the restatement in fp32 and of the kernel; the test's bar is 16 x the former."""
    import numpy as np
    import torch
    from tests import pitch_ref
    y = pitch_ref.glide(HOP * 120 + 77, np.random.default_rng(0))
    ref, margin = pitch_ref.yin(y)
    r32, _ = pitch_ref.yin(y, dtype=np.float32)
    g = pe(torch.from_numpy(y).to(dev).unsqueeze(0))[0].cpu().numpy().astype(np.float64)
    ok = margin >= 1e-4
    v = ok & (ref > 0)
    e32 = float(np.max(np.abs(r32[v & (r32 > 0)] / ref[v & (r32 > 0)] - 1)))
    return {"case": "composite signal, hop * 120 + 77 samples, default_rng(0)", "frames": int(len(ref)), "margin": 1e-4,
            "share_left_out": round(float((~ok).mean()), 4), "voicing_disagreements_on_the_rest": int((ok & ((g > 0) != (ref > 0))).sum()),
            "fp32_numpy_max_rel_dev": e32, "kernel_max_rel_dev": float(np.max(np.abs(g[v] / ref[v] - 1))), "bar_16x_fp32_numpy": 16 * e32}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_time.json"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (for a profiler run)")
    args = ap.parse_args()
    import numpy as np
    lens, wavs = signals()
    host_s, host_f0 = (None, None) if args.no_host else host_baseline(wavs, min(args.procs, 16))
    import torch
    from tests import pitch_ref
    from tts_king_amd import lib, ops
    from tts_king_amd.audio import PitchExtractor, TacotronSTFT
    dev = "cuda:0"
    pe = PitchExtractor(22050, HOP)
    stft = TacotronSTFT(1024, HOP, 1024, 80, 22050, 0, 8000, device=dev)
    ys = [torch.from_numpy(w).to(dev).unsqueeze(0) for w in wavs]
    rng = np.random.default_rng(0)
    durs = []
    for T in lens:                                  # about 8 frames per phoneme, summing to T
        cuts = np.sort(rng.choice(np.arange(1, T), size=T // 8, replace=False))
        durs.append(np.diff(np.concatenate([[0], cuts, [T]])).astype(np.int32))
    f0s = [pe(y) for y in ys]
    ens = [stft.mel_spectrogram(y)[1] for y in ys]
    dur_t = [torch.from_numpy(d).to(dev).unsqueeze(0) for d in durs]
    Tn = [torch.tensor([f.shape[1]], dtype=torch.int32, device=dev) for f in f0s]
    Ln = [torch.tensor([len(d)], dtype=torch.int32, device=dev) for d in durs]
    ld = max(len(w) for w in wavs)
    batch = torch.zeros(len(wavs), ld, device=dev)
    for i, w in enumerate(wavs):
        batch[i, :len(w)] = torch.from_numpy(w)
    blens = torch.tensor([len(w) for w in wavs], dtype=torch.int32, device=dev)
    stages = {
        "pitch_extractor_32_calls": lambda: [pe(y) for y in ys],
        "tacotron_stft_32_calls": lambda: [stft.mel_spectrogram(y) for y in ys],
        "phoneme_prosody_32_calls": lambda: [ops.phoneme_prosody(f, e, d, t, l) for f, e, d, t, l in zip(f0s, ens, dur_t, Tn, Ln)],
        "pitch_yin_one_ragged_launch": lambda: pe(batch, blens),
    }
    for fn in stages.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in stages}
    for _ in range(args.reps):
        for k, fn in stages.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "reps": args.reps, "utterances": len(lens),
              "frames": int(sum(1 + len(w) // HOP for w in wavs)), "lens_frames": lens,
              "unit": "ms of device time between two HIP events around the stage, median over repeats with the stages alternating",
              "stages": {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                         for k, v in times.items()}}
    # what the YIN launch reaches: every frame does W * 4 * NG (sample, lag) pairs, one subtract and one fused multiply-add each,
    # and reads two 16-byte LDS words per lane per 16 pairs
    frames, W, NG = result["frames"], pe.window, pe.tau_max // 4 + 1
    pairs = frames * W * 4 * NG
    t = 1e-3 * result["stages"]["pitch_yin_one_ragged_launch"]["median_ms"]
    result["pitch_yin_rates"] = {"sample_lag_pairs": pairs, "vector_ops_per_s": round(2 * pairs / t, 0), "flop_per_s_counting_fma_as_2": round(3 * pairs / t, 0),
                                 "lds_read_bytes_per_s": round(pairs / 16 * 32 / t, 0),
                                 "active_lanes_of_256": NG * min(256 // NG, W // 4)}
    if host_s is not None:
        result["accuracy"] = accuracy(pe, dev)
        got = [pe(y)[0].cpu().numpy() for y in ys]
        agree = float(np.mean([np.mean((g > 0) == (h > 0)) for g, h in zip(got, host_f0)]))
        t0 = time.perf_counter()
        for f, e, d in zip(f0s, ens, durs):
            pitch_ref.phoneme_prosody(f[0].cpu().numpy(), e[0].cpu().numpy(), d)
        result["host"] = {"what": "tests/pitch_ref.py in fp64 on %d processes of this host, the same arrays" % min(args.procs, 16),
                          "yin_s": round(host_s, 3), "phoneme_prosody_one_process_s": round(time.perf_counter() - t0, 4),
                          "yin_host_over_device_32_calls": round(1e3 * host_s / result["stages"]["pitch_extractor_32_calls"]["median_ms"], 1),
                          "frames_with_the_same_voicing_decision": round(agree, 5)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
