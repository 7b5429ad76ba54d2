"""Time waveforms at the caller's sample rate against the native-rate call on one MI355X.

The workloads of tools/window_vocoder_time.py (8 and 32 utterances of 150-900 frames), through HIFIapi.generate_ragged with every
graph captured, the native rate and 8, 16 and 48 kHz alternating in one process, warm, every call ending in its device-to-host copy:

    python tools/resample_time.py --out profiles/resample_time.json

Writes, per workload and rate, the median and minimum in ms, the time added to the native-rate call of the same process, the bytes
of the device-to-host copy, and -- where scipy imports -- what `scipy.signal.resample_poly` on the native-rate int16 arrays costs on
this host's CPU, which is what a caller does without `sample_rate=`.  Also the structure: the launches of one eager ragged call at
the native rate and at 16 kHz, counted at the library's entry points (the difference must be ttsk_resample, once).
"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RATES = (None, 8000, 16000, 48000)


class CountingLib:
    """Stands in for the loaded library: counts, per entry point, the calls whose last argument is the current stream's handle."""

    def __init__(self, real, counts):
        self.__dict__["_real"], self.__dict__["_counts"] = real, counts

    def __setattr__(self, name, value):
        setattr(self._real, name, value)

    def __getattr__(self, name):
        import torch
        fn, counts = getattr(self._real, name), self._counts

        def forward(*args):
            last = args[-1] if args else None
            last = getattr(last, "value", last)
            if type(last) is int and last == torch.cuda.current_stream().cuda_stream:
                counts[name] = counts.get(name, 0) + 1
            return fn(*args)
        return forward


def launches(model, mels, rate):
    """Entry-point calls of one eager `forward_ragged_flat` (int16), on a stream of its own so that a host-only call's trailing 0 is
    no stream handle; the call before it is not counted (weight packing, the filter's upload)."""
    import torch
    from tts_king_amd import lib
    counts, real = {}, lib.load()
    with torch.cuda.stream(torch.cuda.Stream()):
        model.forward_ragged_flat(mels, False, 32768.0, rate)
        torch.cuda.synchronize()
        lib._lib = CountingLib(real, counts)
        try:
            model.forward_ragged_flat(mels, False, 32768.0, rate)
        finally:
            lib._lib = real
        torch.cuda.synchronize()
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.json"))
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    import torch
    from hifiapi import HIFIapi
    from tools.window_vocoder_time import workloads
    from tts_king_amd import lib, resample
    from tts_king_amd.config import default_config
    from tts_king_amd.synthetic import make_mel
    try:
        from scipy.signal import resample_poly
    except ImportError:
        resample_poly = None
    c = copy.deepcopy(default_config())
    c.model_config["vocoder"]["use_cpu"] = False
    c.mi355x["hip_graph"] = True
    api = HIFIapi(c, "cuda:0")
    native = int(c.hifi.sampling_rate)
    result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(), "reps": args.reps, "native_rate": native,
              "unit": "ms per call, host clock around HIFIapi.generate_ragged (graph replayed, device-to-host copy included)",
              "filters": {}, "workloads": {}}
    for rate in RATES[1:]:
        L, M, P, C, table = resample.design(native, rate)
        result["filters"][str(rate)] = {"L": L, "M": M, "P": P, "C": C, "table_bytes": int(table.nbytes)}
    for name, lens in workloads().items():
        if len(lens) < 2:
            continue
        mels = [make_mel(1, T, seed=T)[0].to("cuda:0") for T in lens]
        variants = {str(r or native): (lambda r=r: api.generate_ragged(mels, sample_rate=r)) for r in RATES}
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
        row = {"lens": lens, "frames": sum(lens), "graphs": len(api._synth._rag)}
        base = statistics.median(times[str(native)])
        wavs = variants[str(native)]()
        for r in RATES:
            k = str(r or native)
            flat, plan, _ = api._synth.wav_ragged_flat(mels, False, 32768.0, r)
            row[k] = {"median_ms": round(statistics.median(times[k]), 4), "min_ms": round(min(times[k]), 4),
                      "added_to_native_ms": round(statistics.median(times[k]) - base, 4), "d2h_bytes": flat.numel() * flat.element_size(),
                      "samples": sum(resample.out_len(256 * T, *resample.factor(native, r or native)) for T in lens)}
            if r is not None and resample_poly is not None:
                g = math.gcd(native, r)
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    for w in wavs:
                        resample_poly(w.reshape(-1), r // g, native // g)
                    host.append(1e3 * (time.perf_counter() - t0))
                row[k]["scipy_resample_poly_on_host_ms"] = round(statistics.median(host), 4)
        # the launch alone: HIP events around 20 back-to-back eager launches on this workload's native-rate fp32 buffer
        from tts_king_amd import ops
        flat32, plan, _ = api.model.forward_ragged_flat(mels)
        for r in RATES[1:]:
            filt = api.model.resampler(r)
            sg = api.model.plan_resample(plan, filt)
            segs = torch.from_numpy(sg.table).to(flat32.device)
            out = torch.empty(sg.n_dst, dtype=torch.int16, device=flat32.device)
            ops.resample(flat32, segs, filt, out=out, int16_scale=32768.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                ops.resample(flat32, segs, filt, out=out, int16_scale=32768.0)
            e1.record()
            torch.cuda.synchronize()
            row[str(r)]["kernel_us"] = round(1e3 * e0.elapsed_time(e1) / 20, 2)
        result["workloads"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if isinstance(v, dict)}), flush=True)
    # structure: what 16 kHz adds to one ragged call
    lens = workloads()["8_utterances_150_900"]
    mels = [make_mel(1, T, seed=T)[0].to("cuda:0") for T in lens]
    a, b = launches(api.model, mels, None), launches(api.model, mels, 16000)
    added = {k: b.get(k, 0) - a.get(k, 0) for k in sorted(set(a) | set(b)) if b.get(k, 0) != a.get(k, 0)}
    result["launches"] = {"native": sum(a.values()), "16000": sum(b.values()), "added": added}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["launches"]))


if __name__ == "__main__":
    main()
