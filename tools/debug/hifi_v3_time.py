"""HiFi-GAN V3 generator (ResBlock2, the published config_v3 through the `hifi:` keys): the fused route (one ttsk_hifi_resblock2 launch per
block, csrc/resblock2.hip) against the conv-by-conv route (`Generator.resblock2_fused = False`: implicit-GEMM convs, the upsampler's lrelu
copy, avg3), alternated in one process after warm-up, timed with HIP events on eager launches.  Prints per shape both routes' median ms
per forward, the per-stage split (Generator._stage_marks) and the waveform rel-RMS between the routes (bar: 2e-3), as JSON lines.

    python tools/debug/hifi_v3_time.py [--iters N] [--fused-only]

--fused-only runs the fused route alone (no comparison): the launch sequence for a kernel trace,
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/debug/hifi_v3_time.py --iters 1 --warmup 1 --fused-only"""
import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))     # the repository root
from tts_king_amd.config import default_config  # noqa: E402
from tts_king_amd.hifigan import Generator  # noqa: E402
from tts_king_amd.synthetic import make_mel  # noqa: E402

V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])


def v3_generator(dev, seed=11):
    cfg = copy.deepcopy(default_config())
    for k, v in V3.items():
        cfg.hifi[k] = v
    gen = Generator(cfg.hifi)
    gen.reset_parameters(seed)
    gen.to(dev)
    gen.remove_weight_norm()
    return gen.eval()


def timed(gen, mel):
    """One forward: total device ms and ms per stage (between consecutive stage marks)."""
    gen._stage_marks = marks = []
    try:
        y = gen(mel)
    finally:
        gen._stage_marks = None
    torch.cuda.synchronize()
    stages = {n1: e0.elapsed_time(e1) for (n0, e0), (n1, e1) in zip(marks[:-1], marks[1:])}
    return y, marks[0][1].elapsed_time(marks[-1][1]), stages


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    gen = v3_generator(dev)
    for B, T in ((8, 384), (1, 448)):
        mel = make_mel(B, T, seed=7).to(dev)
        times = {True: [], False: []}
        split = {True: {}, False: {}}
        outs = {}
        for it in range(args.warmup + args.iters):
            for fused in ((True,) if args.fused_only else (True, False)):
                gen.resblock2_fused = fused
                y, ms, st = timed(gen, mel)
                outs[fused] = y
                if it >= args.warmup:
                    times[fused].append(ms)
                    for k, v in st.items():
                        split[fused].setdefault(k, []).append(v)
        gen.resblock2_fused = True
        if args.fused_only:
            print(json.dumps({"B": B, "T": T, "fused_ms": round(med(times[True]), 4),
                              "fused_stages_ms": {k: round(med(v), 4) for k, v in split[True].items()}}))
            continue
        a, b = outs[True].double(), outs[False].double()
        r = float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())
        rec = {"B": B, "T": T, "fused_ms": round(med(times[True]), 4), "conv_by_conv_ms": round(med(times[False]), 4),
               "speedup": round(med(times[False]) / med(times[True]), 3),
               "fused_stages_ms": {k: round(med(v), 4) for k, v in split[True].items()},
               "conv_by_conv_stages_ms": {k: round(med(v), 4) for k, v in split[False].items()},
               "rel_rms_between_routes": r, "agree": r <= 2e-3, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec))
        if r > 2e-3:
            sys.exit("routes disagree: rel-RMS %.3e > 2e-3" % r)


if __name__ == "__main__":
    main()
