"""Time the Griffin-Lim loop (tts_king_amd/audio.py: griffin_lim on csrc/griffinlim.hip) on one MI355X.

32 synthetic utterances of 150-900 frames (the lengths of tools/window_vocoder_time.py) at the shipped STFT (1024 / 256 / 1024),
60 iterations, magnitudes of a chirp plus noise, phases from a seed:

    python tools/griffinlim_time.py --out profiles/griffinlim_time.json

Timed, as device time between two HIP events, medians over repeats in which the variants alternate in one process:
  batched      one griffin_lim call on the (32, 513, T_max) batch with `lens`
  solo_loop    32 griffin_lim calls, one per utterance
  torch_solo   the same iteration written with torch.stft / torch.istft / torch.polar(m, angle(Z)) on the same device, 32 calls
  torch_padded that iteration on the padded batch as one call (it has no `lens`: the short rows iterate on their padding too, so it
               is not the same computation; it shows what batching alone buys torch)
Also: launches of this library's kernels per batched call (counted by tts_king_amd.ops; the few torch kernels `griffin_lim` issues
once per call -- two layout copies, the `lens` upload -- are not in that count), device time per iteration = batched / 60, and the spectral convergence
of utterance 0 after the 60 iterations from both implementations.  A record, not a pass bar.  A variant that cannot run on the
machine is written as "not measured" with the reason."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_FFT, HOP, WIN, ITERS = 1024, 256, 1024, 60


def targets():
    """(frames per utterance, [m (513, T) float32], [phase0 (513, T) float32])."""
    import numpy as np
    from tests import griffinlim_ref as R
    from tools.window_vocoder_time import workloads
    lens = workloads()["32_utterances_150_900"]
    ms, ps = [], []
    for T in lens:
        m = np.abs(R.stft(R.signal(HOP * (T - 1), T), N_FFT, HOP, WIN)).astype(np.float32)
        ms.append(m)
        ps.append((np.random.RandomState(T).rand(*m.shape) * 2 * np.pi).astype(np.float32))
    return lens, ms, ps


def torch_griffin_lim(m, phase0, window, n_iters):
    import torch
    n = HOP * (m.shape[-1] - 1)
    kw = dict(n_fft=N_FFT, hop_length=HOP, win_length=WIN, window=window, center=True)
    x = torch.istft(torch.polar(m, phase0), length=n, **kw)
    for _ in range(n_iters):
        z = torch.stft(x, pad_mode="reflect", return_complex=True, **kw)
        x = torch.istft(torch.polar(m, torch.angle(z)), length=n, **kw)
    return x


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "griffinlim_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=ITERS)
    args = ap.parse_args()
    import numpy as np
    import torch
    from tests import griffinlim_ref as R
    from tts_king_amd import lib, ops
    from tts_king_amd.audio import STFT, griffin_lim
    dev = "cuda:0"
    lens, ms, ps = targets()
    s = STFT(N_FFT, HOP, WIN)
    md = [torch.from_numpy(m).to(dev).unsqueeze(0) for m in ms]
    pd = [torch.from_numpy(p).to(dev).unsqueeze(0) for p in ps]
    Tm = max(lens)
    mb = torch.zeros(len(lens), N_FFT // 2 + 1, Tm, device=dev)
    pb = torch.zeros_like(mb)
    for i, T in enumerate(lens):
        mb[i, :, :T], pb[i, :, :T] = md[i][0], pd[i][0]
    window = torch.hann_window(WIN, periodic=True, device=dev)
    variants = {
        "batched": lambda: griffin_lim(mb, s, args.iters, phase0=pb, lens=lens),
        "solo_loop": lambda: [griffin_lim(m, s, args.iters, phase0=p) for m, p in zip(md, pd)],
        "torch_solo": lambda: [torch_griffin_lim(m, p, window, args.iters) for m, p in zip(md, pd)],
        "torch_padded": lambda: torch_griffin_lim(mb, pb, window, args.iters),
    }
    not_measured = {}
    for k in list(variants):
        try:
            for _ in range(2):
                variants[k]()
            torch.cuda.synchronize()
        except Exception as e:            # e.g. an FFT library that is not installed: recorded, not estimated
            not_measured[k] = "not measured: %s: %s" % (type(e).__name__, str(e)[:200])
            del variants[k]
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    ops.LAUNCH_COUNTS = {}
    out = variants["batched"]()
    torch.cuda.synchronize()
    launches, ops.LAUNCH_COUNTS = ops.LAUNCH_COUNTS, None
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "reps": args.reps, "iterations": args.iters,
              "stft": [N_FFT, HOP, WIN], "utterances": len(lens), "frames": int(sum(lens)), "lens_frames": lens,
              "unit": "ms of device time between two HIP events around the call(s), median over repeats with the variants alternating",
              "variants": {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
                           for k, v in times.items()},
              "launches_per_batched_call": launches, "launches_per_iteration": 1}
    result["variants"].update(not_measured)
    tb = result["variants"]["batched"]["median_ms"]
    result["batched_ms_per_iteration"] = round(tb / max(args.iters, 1), 4)
    result["batched_us_per_frame_and_iteration"] = round(1e3 * tb / max(args.iters, 1) / sum(lens), 4)
    for k in ("solo_loop", "torch_solo", "torch_padded"):
        if k in times:
            result["%s_over_batched" % k] = round(result["variants"][k]["median_ms"] / tb, 2)
    m0 = ms[0].astype(np.float64)
    conv = {"kernel": R.convergence(out[0, :HOP * (lens[0] - 1)].cpu().numpy(), m0, N_FFT, HOP, WIN)}
    if "torch_solo" in variants:
        conv["torch"] = R.convergence(torch_griffin_lim(md[0], pd[0], window, args.iters)[0].cpu().numpy(), m0, N_FFT, HOP, WIN)
    result["spectral_convergence_utterance_0"] = {k: round(v, 5) for k, v in conv.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
