#!/usr/bin/env python3
"""GPU box: the graph-replayed train step of the plain model against the CWT model (model_config.use_cwt: True), alternated in ONE
process on one box (boxes differ by several per cent in clock: only numbers from one run compare, cf. tools/ab_libs.sh).

Both models are built as bench.py builds its headline model (B = 16, L = 64, seed 1234, grad_acc_step 1, dropout on, one captured
hipGraph per model; the CWT batch carries seeded CWT targets, the CWT model's heads are made live as in the parity fixtures).  After
the warm-up the two graphs take turns in blocks of at least `--block-seconds` of replays, each block timed with device events;
printed: the per-block ms/step, both medians, the spread (max - min over a model's blocks) and the difference.

    python tools/cwt_step_time.py [--rounds 5] [--block-seconds 1.0] [--launches]

--launches: instead of timing, run `--steps` eager steps of the model(s) and stop — for a kernel trace in a run of its own
(`rocprofv3 --kernel-trace --stats -- python tools/cwt_step_time.py --launches --only plain --steps 2`, again with --steps 4: the
difference of the two kernel counts / 2 is the launch count of a step).
Writes profiles/cwt_step_time.json (`--out`; source fingerprint alongside) unless --no-write.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(use_cwt, dev):
    from tts_king_amd.config import default_config
    from tts_king_amd.fastspeech2 import FastSpeech2
    from tts_king_amd.graph import make_enqueue
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.optimizer import ScheduledOptim
    from tts_king_amd.synthetic import make_batch
    from tts_king_amd.train_step import to_device
    cfg = copy.deepcopy(default_config())
    cfg.train_config["optimizer"]["grad_acc_step"] = 1
    cfg.model_config["use_cwt"] = bool(use_cwt)
    model = FastSpeech2(cfg.preprocess_config, cfg.model_config, 65, device=dev, seed=1234).train()
    if use_cwt:
        # with the seeded fill alone pitch_std's last ReLU is dead for every row: make both heads' last layer positive (as the parity
        # fixtures do), so that the timed step runs the heads' whole backward
        with torch.no_grad():
            for h in ("pitch_mean", "pitch_std"):
                w = model.get("variance_adaptor.%s.linear.weight" % h)
                w.copy_(0.25 * w.abs())
                model.get("variance_adaptor.%s.linear.bias" % h).fill_(0.25)
        model.mark_dirty()
    opt = ScheduledOptim(model, cfg.train_config, cfg.model_config, 0)
    loss_fn = FastSpeech2Loss(cfg.preprocess_config, cfg.model_config)
    cpu_batch = list(make_batch(16, 64, seed=1234))
    if use_cwt:        # seeded CWT targets instead of make_batch's zeros / 0 / 1
        g = torch.Generator().manual_seed(1234)
        cpu_batch[12], cpu_batch[13], cpu_batch[14] = torch.randn(16, 64, 11, generator=g), 5.0 + 0.3 * torch.randn(16, generator=g), \
            0.5 + torch.rand(16, generator=g)
    batch = to_device(tuple(cpu_batch), dev)
    return model, make_enqueue(model, opt, cfg, loss_fn), batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--only", choices=("plain", "cwt"))
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cwt_step_time.json"))
    ap.add_argument("--steps", type=int, default=2, help="--launches: eager steps per model")
    args = ap.parse_args()
    from tts_king_amd import lib
    from tts_king_amd.graph import GraphedTrainStep
    lib.load()
    dev = "cuda:0"
    names = [n for n in ("plain", "cwt") if args.only in (None, n)]
    built = {n: build(n == "cwt", dev) for n in names}
    if args.launches:
        # --steps eager steps per model: the difference between the kernel counts of two profiled runs (say 2 and 4 steps) divided by
        # the difference in steps is the launch count of one step (construction and the first step's planning drop out)
        for n in names:
            _, enq, batch = built[n]
            for _ in range(args.steps):
                enq(batch)
            torch.cuda.synchronize()
            print("launches: ran %d eager steps of the %s model" % (args.steps, n))
        return
    graphs = {}
    for n in names:
        _, enq, batch = built[n]
        graphs[n] = GraphedTrainStep(enq, batch, warmup=2)
        for _ in range(args.warmup):
            graphs[n].run()
    torch.cuda.synchronize()
    blocks = {n: [] for n in names}
    for r in range(args.rounds):
        for n in names:
            g = graphs[n]
            iters = 50
            while True:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    g.run()
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 1000.0 * args.block_seconds:
                    break
                iters = int(iters * max(1.5, 1100.0 * args.block_seconds / max(ms, 1.0)))
            blocks[n].append(ms / iters)
            print("round %d %-5s %d replays %.4f ms/step" % (r, n, iters, ms / iters), flush=True)
    res = {"source_fingerprint": lib.source_fingerprint(), "shape": {"B": 16, "L": 64}, "block_seconds": args.block_seconds}
    for n in names:
        res[n] = {"median_ms": statistics.median(blocks[n]), "spread_ms": max(blocks[n]) - min(blocks[n]), "blocks_ms": blocks[n]}
    if len(names) == 2:
        res["cwt_minus_plain_ms"] = res["cwt"]["median_ms"] - res["plain"]["median_ms"]
    print(json.dumps(res))
    if not args.no_write:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
