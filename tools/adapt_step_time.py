#!/usr/bin/env python3
"""GPU box: the graph-replayed train step with everything trained against three speaker-adaptation steps (FastSpeech2.set_trainable),
alternated in ONE process on one box (boxes differ by several per cent in clock: only numbers from one run compare, cf.
tools/cwt_step_time.py).

Every model is built as bench.py builds its headline model (B = 16, L = 64, T = 423, seed 1234, grad_acc_step 1, dropout on) and runs
through TrainEngine with hip_graph on: the first step of the shape eager, the second captured, then replays.  After the warm-up the
four engines take turns in blocks of at least `--block-seconds` of replays, each block timed with device events; printed and written:
per-block ms/step, medians, spreads (max - min over a configuration's blocks), the launches of one traced eager step (calls of library
entry points that take a stream, traced through a stand-in for the loaded library; an entry point may be more than one kernel: the
optimizer step is two), and whether each subset step beats the full step by more than the full step's own block-to-block spread.

    python tools/adapt_step_time.py [--rounds 5] [--block-seconds 1.0]

Writes profiles/adapt_step_time.json (`--out`; source fingerprint alongside) unless --no-write.
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

CONFIGS = [("full", None), ("speaker_emb", ["speaker_emb"]), ("speaker_emb+variance_adaptor", ["speaker_emb", "variance_adaptor"]),
           ("speaker_emb+variance_adaptor+decoder", ["speaker_emb", "variance_adaptor", "decoder"])]


def build(units, dev):
    from tts_king_amd.config import default_config
    from tts_king_amd.engine import TrainEngine
    from tts_king_amd.fastspeech2 import FastSpeech2
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.optimizer import ScheduledOptim
    from tts_king_amd.synthetic import make_batch
    from tts_king_amd.train_step import to_device
    cfg = copy.deepcopy(default_config())
    cfg.train_config["optimizer"]["grad_acc_step"] = 1
    model = FastSpeech2(cfg.preprocess_config, cfg.model_config, 65, device=dev, seed=1234).train()
    model.set_trainable(units)
    opt = ScheduledOptim(model, cfg.train_config, cfg.model_config, 0)
    eng = TrainEngine(model, opt, cfg, FastSpeech2Loss(cfg.preprocess_config, cfg.model_config), hip_graph=True)
    batch = to_device(make_batch(16, 64, seed=1234), dev)
    return eng, batch


def count_launches(eng, batch):
    """Library calls that take the current stream (= kernel launches and the few table uploads) in one eager step of the engine's
    enqueue closure, through a stand-in for the loaded library."""
    import ctypes as C
    from tts_king_amd import lib
    real = lib.load()
    names = []

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def forward(*args):
                last = args[-1] if args else None
                last = last.value if isinstance(last, C.c_void_p) else last
                if type(last) is int and last != 0 and last in streams:
                    names.append(name)
                return fn(*args)
            return forward

        def __setattr__(self, name, value):
            setattr(real, name, value)
    main = torch.cuda.Stream()
    m = eng.model
    with torch.cuda.stream(main):
        enq = eng._enqueue(True, None, None)
        enq(batch)                           # side streams exist after this one
        torch.cuda.synchronize()
        streams = {s.cuda_stream for s in (main, m._dw_side, m._fin_side, m._pred_stream) if s is not None}
        lib._lib = Proxy()
        try:
            enq(batch)
        finally:
            lib._lib = real
        torch.cuda.synchronize()
    eng.optimizer._host_step = eng.optimizer.current_step
    by = {}
    for n in names:
        by[n] = by.get(n, 0) + 1
    return len(names), by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapt_step_time.json"))
    args = ap.parse_args()
    from tts_king_amd import lib
    lib.load()
    dev = "cuda:0"
    built = {n: build(u, dev) for n, u in CONFIGS}
    launches = {}
    for n, _ in CONFIGS:
        eng, batch = built[n]
        launches[n] = count_launches(eng, batch)
        step = 1
        for _ in range(2 + args.warmup):          # eager, capture, replays
            eng.step(batch, step)
            step += 1
        torch.cuda.synchronize()
        assert eng.stats["captured"] == 1 and eng.stats["replayed"] == args.warmup, (n, eng.stats, getattr(eng, "last_capture_error", None))
        print("%-40s %d stream calls per step; engine %s" % (n, launches[n][0], eng.stats), flush=True)
    blocks = {n: [] for n, _ in CONFIGS}
    for r in range(args.rounds):
        for n, _ in CONFIGS:
            eng, batch = built[n]
            iters = 50
            while True:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    eng.step(batch, 1)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 1000.0 * args.block_seconds:
                    break
                iters = int(iters * max(1.5, 1100.0 * args.block_seconds / max(ms, 1.0)))
            blocks[n].append(ms / iters)
            print("round %d %-40s %d replays %.4f ms/step" % (r, n, iters, ms / iters), flush=True)
    res = {"source_fingerprint": lib.source_fingerprint(), "shape": {"B": 16, "L": 64, "T": 423}, "block_seconds": args.block_seconds}
    for n, u in CONFIGS:
        res[n] = {"units": u, "median_ms": statistics.median(blocks[n]), "spread_ms": max(blocks[n]) - min(blocks[n]), "blocks_ms": blocks[n],
                  "stream_calls": launches[n][0], "stream_calls_by_entry_point": dict(sorted(launches[n][1].items()))}
    full = res["full"]
    for n, _ in CONFIGS[1:]:
        res[n]["full_minus_this_ms"] = full["median_ms"] - res[n]["median_ms"]
        res[n]["faster_than_full_by_more_than_its_spread"] = bool(res[n]["full_minus_this_ms"] > full["spread_ms"])
    print(json.dumps(res))
    if not args.no_write:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
