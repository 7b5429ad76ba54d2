"""What the FS2 trainer sustains from a preprocessed directory on one MI355X: the loader route against the resident route.

Writes a synthetic preprocessed directory to a temporary directory (2048 utterances at the benchmark's sizes: 57-64 phonemes, 1-11
frames per phoneme, so a batch of 16 is L = 64, T around 423 — the generator of tests/test_dataset_cpu.py:synthetic_samples scaled up),
builds ONE model / optimizer / TrainEngine, warms every shape's graph, and then alternates, in one process, blocks of steps fed by

  loader      train.py's chain as it is: DataLoader(num_workers=4, groups of batch_size*4) -> collate_fn -> DeviceFeeder
  loader_aa   the same chain a second time (a second DataLoader): the A/A pair that gives the run-to-run spread
  loader_w0   the same chain with num_workers=0 (mi355x.loader_workers: 0): the utterances loaded in the training process itself
  resident    ResidentStore + ResidentLoader (mi355x.resident_data): one ttsk_collate_batch launch per step
  replay      one fixed device batch over and over: the step alone, no data path

every block between two device synchronisations on the host clock, medians over the blocks.  Before a loader block is timed, the
batches its workers prefetched while the other routes ran are pulled and dropped, so the block shows what the chain sustains and not
what it had stored up.  The loader routes also record the host time they spend waiting for each group of four batches (an epoch's
first group apart: a new DataLoader iterator starts new workers, every 128 steps at this size, as in train.py's loop) and inside the
DeviceFeeder, over the whole run.  Then, untimed, one block per route with the launches counted at the library entry points
(ops.LAUNCH_COUNTS) and the host-to-device copies counted where both routes make them (a host tensor's `.to(device)` / `.cuda()` /
`copy_` into a device tensor).

    python tools/resident_data_time.py --out profiles/resident_data_time.json
"""
import argparse
import copy
import json
import os
import shutil
import signal
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_corpus(root, n, seed=9):
    """synthetic_samples (tests/test_dataset_cpu.py) at the benchmark's sizes, written as prepare_data.py lays a directory out."""
    import numpy as np
    from tts_king_amd import text as T
    rng = np.random.RandomState(seed)
    syms = T.symbols()
    for d in ("mel", "energy", "duration", "pitch"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    lines, frames = [], []
    for i in range(n):
        L = int(rng.randint(57, 65))
        dur = rng.randint(1, 12, size=L)
        Tn = int(dur.sum())
        frames.append(Tn)
        spk, b = "spk%d" % (i % 3), "utt%05d" % i
        lines.append("%s|%s|{%s}|raw %d" % (b, spk, " ".join(syms[j][1:] for j in 150 + rng.randint(0, 50, size=L)), i))
        np.save(os.path.join(root, "mel", "%s-mel-%s.npy" % (spk, b)), rng.randn(Tn, 80).astype(np.float32))
        np.save(os.path.join(root, "energy", "%s-energy-%s.npy" % (spk, b)), rng.randn(L).astype(np.float32))
        np.save(os.path.join(root, "duration", "%s-duration-%s.npy" % (spk, b)), dur)
        np.save(os.path.join(root, "pitch", "%s-pitch-%s.npy" % (spk, b)), rng.randn(L).astype(np.float32))
        np.save(os.path.join(root, "pitch", "%s-cwt-pitch-%s.npy" % (spk, b)), rng.randn(L, 11).astype(np.float32))
        np.save(os.path.join(root, "pitch", "%s-pitch-mean-%s.npy" % (spk, b)), np.float32(rng.randn()))
        np.save(os.path.join(root, "pitch", "%s-pitch-std-%s.npy" % (spk, b)), np.float32(abs(rng.randn()) + 0.1))
    for name, rows in (("train.txt", lines), ("val.txt", lines[:64])):
        with open(os.path.join(root, name), "w", encoding="utf-8") as f:
            f.write("\n".join(rows) + "\n")
    with open(os.path.join(root, "speakers.json"), "w") as f:
        f.write('{"spk0": 0, "spk1": 1, "spk2": 2}')
    shutil.copy(os.path.join(ROOT, "pretrained", "stats.json"), os.path.join(root, "stats.json"))
    return frames


class H2DCounter:
    """Counts host-to-device copies made through Tensor.to / Tensor.cuda / Tensor.copy_ while active."""

    def __enter__(self):
        import torch
        self.n, self.torch = 0, torch
        self.keep = (torch.Tensor.to, torch.Tensor.cuda, torch.Tensor.copy_)
        to, cuda, copy_ = self.keep
        me = self

        def counted_to(t, *a, **kw):
            out = to(t, *a, **kw)
            me.n += int((not t.is_cuda) and out.is_cuda)
            return out

        def counted_cuda(t, *a, **kw):
            me.n += int(not t.is_cuda)
            return cuda(t, *a, **kw)

        def counted_copy(t, src, *a, **kw):
            me.n += int(t.is_cuda and torch.is_tensor(src) and not src.is_cuda)
            return copy_(t, src, *a, **kw)

        torch.Tensor.to, torch.Tensor.cuda, torch.Tensor.copy_ = counted_to, counted_cuda, counted_copy
        return self

    def __exit__(self, *exc):
        self.torch.Tensor.to, self.torch.Tensor.cuda, self.torch.Tensor.copy_ = self.keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_data_time.json"))
    ap.add_argument("--utterances", type=int, default=2048)
    ap.add_argument("--block", type=int, default=200, help="steps per timed block")
    ap.add_argument("--reps", type=int, default=7, help="timed blocks per route")
    ap.add_argument("--warmup", type=int, default=300, help="steps per route before anything is timed")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the whole run is ended (SIGALRM)")
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    import torch
    from torch.utils.data import DataLoader, RandomSampler
    from tts_king_amd import lib, ops
    from tts_king_amd.config import default_config
    from tts_king_amd.dataset import Dataset, DeviceFeeder
    from tts_king_amd.engine import TrainEngine
    from tts_king_amd.loss import FastSpeech2Loss
    from tts_king_amd.resident import ResidentLoader, ResidentStore
    from tts_king_amd.train_step import get_model
    if not torch.cuda.is_available():
        raise SystemExit("resident_data_time needs an MI355X: there is no CPU path and nothing to time without one")
    dev = "cuda:0"
    root = tempfile.mkdtemp(prefix="resident_data_time_")
    try:
        t0 = time.perf_counter()
        frames = write_corpus(root, args.utterances)
        t_write = time.perf_counter() - t0
        cfg = copy.deepcopy(default_config())
        cfg.preprocess_config.path.preprocessed_path = root
        cfg.train_config["optimizer"]["batch_size"] = 16
        bs = 16
        mi = cfg.mi355x
        bucket = (int(mi.get("l_bucket", 8)), int(mi.get("t_bucket", 32)), int(cfg.model_config["max_seq_len"]))
        model, optimizer = get_model(cfg, dev, train=True)
        engine = TrainEngine(model, optimizer, cfg, FastSpeech2Loss(cfg.preprocess_config, cfg.model_config))
        dataset = Dataset("train.txt", cfg.preprocess_config, cfg.train_config, sort=True, drop_last=True)

        # host seconds inside the loader routes, by worker count: waiting for a group of 4 batches (an epoch's first, when the workers
        # start, apart from the others) and inside the DeviceFeeder (staging, the H2D copy, its stream and event waits), with the batches fed
        host = {w: {"epoch_start": [], "group": [], "feeder_s": 0.0, "batches": 0} for w in {args.workers, 0}}

        def loader_route(workers):
            loader = DataLoader(dataset, batch_size=bs * 4, shuffle=True, collate_fn=dataset.collate_fn, num_workers=workers)
            h = host[workers]
            while True:
                t0, kind = time.perf_counter(), "epoch_start"
                for batchs in loader:                                 # (a new iterator, and new workers, every epoch: as train.py's loop)
                    h[kind].append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    for batch in DeviceFeeder(batchs, dev, bucket=bucket):
                        h["feeder_s"] += time.perf_counter() - t0
                        h["batches"] += 1
                        yield batch
                        t0 = time.perf_counter()
                    h["feeder_s"] += time.perf_counter() - t0
                    t0, kind = time.perf_counter(), "group"

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = ResidentStore("train.txt", cfg.preprocess_config, cfg.train_config, dev, max_gb=float(mi.get("resident_max_gb", 32)))
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0

        def resident_route():
            loader = ResidentLoader(store, bs, 4, sort=True, drop_last=True, sampler=RandomSampler(store), bucket=bucket)
            while True:
                yield from loader

        def replay_route():
            batch = store.batch(list(range(bs)), bucket)
            while True:
                yield batch

        routes = {"loader": loader_route(args.workers), "loader_aa": loader_route(args.workers), "loader_w0": loader_route(0),
                  "resident": resident_route(), "replay": replay_route()}
        stored_up = args.workers * 2 * 4 + args.workers * 4         # batches the workers hold ready (prefetch_factor 2) or have in hand
        step = [1]

        def run(name, n, drain=True):
            it = routes[name]
            if drain and name in ("loader", "loader_aa"):
                for _ in range(stored_up):
                    next(it)
            engine.wait()
            t0 = time.perf_counter()
            for _ in range(n):
                engine.step(next(it), step[0])
                step[0] += 1
            engine.wait()
            return 1e3 * (time.perf_counter() - t0) / n

        for name in routes:                                         # every shape eager once, captured once, then replayed
            run(name, args.warmup, drain=False)
        warm = dict(engine.stats)
        times = {k: [] for k in routes}
        for _ in range(args.reps):
            for name in routes:
                times[name].append(run(name, args.block))
        timed = {k: engine.stats[k] - warm[k] for k in ("eager", "captured", "replayed")}
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = abs(med["loader"] - med["loader_aa"])
        result = {"device": torch.cuda.get_device_name(0), "sources": lib.source_fingerprint(),
                  "unit": "ms per step: host clock around a block of steps between two device synchronisations, median over the blocks",
                  "corpus": {"utterances": args.utterances, "phonemes": "57-64", "frames_mean": round(sum(frames) / len(frames), 1),
                             "frames_max": max(frames), "write_s": round(t_write, 2)},
                  "batch_size": bs, "bucket": list(bucket), "workers": args.workers, "block_steps": args.block, "blocks": args.reps,
                  "warmup_steps_per_route": args.warmup, "graph_steps_while_timed": timed,
                  "ms_per_step": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4), "blocks": [round(x, 4) for x in v]}
                                  for k, v in times.items()},
                  "aa_spread_ms": round(spread, 4),
                  "resident_minus_loader_ms": round(med["resident"] - med["loader"], 4),
                  "resident_not_slower_than_loader_by_more_than_the_spread": bool(med["resident"] <= med["loader"] + spread),
                  "loader_host_time": {"workers_%d" % w: {
                      "batches": h["batches"], "device_feeder_ms_per_batch": round(1e3 * h["feeder_s"] / max(h["batches"], 1), 3),
                      "dataloader_wait_ms_per_batch": round(1e3 * (sum(h["epoch_start"]) + sum(h["group"])) / max(h["batches"], 1), 3),
                      "epoch_start_wait_s": {"n": len(h["epoch_start"]), "median": round(statistics.median(h["epoch_start"] or [0]), 4)},
                      "group_wait_s": {"n": len(h["group"]), "median": round(statistics.median(h["group"] or [0]), 4)}} for w, h in host.items()},
                  "loader_steps_per_epoch": len(dataset) // (bs * 4) * 4 + (len(dataset) % (bs * 4)) // bs,
                  "store": {"load_s": round(t_load, 3), "nbytes": int(store.nbytes), "utterances": len(store)}}
        print(json.dumps({k: v["median"] for k, v in result["ms_per_step"].items()}), "A/A spread", result["aa_spread_ms"], flush=True)
        # untimed: launches at the library entry points and host-to-device copies, one block per route, inside one epoch
        counts = {}
        n = max(1, min(args.block, 64, len(store) // bs - 1))
        routes["resident"] = resident_route()                        # a fresh epoch of 128 steps: the counted block lies inside it
        for name in routes:
            it = routes[name]
            next(it)                                                  # (the resident epoch's one upload, its index plan, happens here)
            ops.LAUNCH_COUNTS = {}
            with H2DCounter() as h:
                for _ in range(n):
                    engine.step(next(it), step[0])
                    step[0] += 1
            engine.wait()
            counts[name] = {"steps": n, "collate_batch_launches": ops.LAUNCH_COUNTS.get("collate_batch", 0), "h2d_copies": h.n}
            ops.LAUNCH_COUNTS = None
        result["counts"] = counts
        print(json.dumps(counts), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        for it in routes.values():
            it.close()                                                # (ends the DataLoader workers)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
