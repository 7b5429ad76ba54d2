#!/usr/bin/env python3
"""A/B of two checkouts of this repository on one MI355X, for a change that moves no arithmetic (the FastSpeech2 kernel plan): what
can move is host time per eager step.  An A/A pair of the parent first (its spread), then parent and new alternated, 5 processes each.
Per process, in the checkout under test:

  (a) bench.py's replayed FS2 step                       ms_per_step
  (b) the same eager (--no-graph)                        ms_per_step_eager
  (c) one eager `_forward` + `backward_native` at the shipped bench shape: host microseconds (perf_counter around the calls,
      synchronised afterwards), median of 60             host_us_fwd_bwd

    python tools/fs2_plan_ab.py --parent <checkout of the parent, built> --new <checkout of the new tree, built> \\
        --parent-commit <hash> --out profiles/fs2_plan_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

BENCH = ["--gpus", "1", "--steps", "100", "--warmup", "20", "--no-hifi", "--no-mel", "--no-e2e", "--no-cpu-baseline", "--no-roofline", "--no-extra"]
KEYS = ("ms_per_step", "ms_per_step_eager", "host_us_fwd_bwd")


def host_us(tree):
    """(c), in this process, on the package of `tree`."""
    sys.path.insert(0, tree)
    import torch
    from tts_king_amd import ops
    from tts_king_amd.config import default_config
    from tts_king_amd.fastspeech2 import FastSpeech2
    from tts_king_amd.synthetic import make_batch
    cfg = default_config()
    m = FastSpeech2(cfg.preprocess_config, cfg.model_config, 65, device="cuda:0", seed=7).train()
    b = make_batch(16, 64, seed=1234)               # bench.py's default batch
    d = [t.to("cuda:0") if torch.is_tensor(t) else t for t in b]
    times = []
    with torch.no_grad():
        for i in range(70):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, ctx = m._forward(True, d[2], d[3], d[4], int(b[5]), d[7], b[8], d[9], d[10], d[11], 1.0, 1.0, 1.0)
            t1 = time.perf_counter()
            _, dmel_sum, dpost, dp, de, dd = ops.fs2_loss(out[0], out[8], d[6], d[7], out[1], out[2], out[3], d[11], d[9], d[10], d[4], grad_scale=1.0)
            t2 = time.perf_counter()
            m.backward_native(ctx, dmel_sum, dpost, dp, de, dd, accumulate=False)
            t3 = time.perf_counter()
            torch.cuda.synchronize()
            if i >= 10:
                times.append(1e6 * ((t1 - t0) + (t3 - t2)))
    print(json.dumps({"host_us_fwd_bwd": statistics.median(times)}))


def last_json(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def one_process_set(tree):
    run = {}
    for key, extra in (("ms_per_step", []), ("ms_per_step_eager", ["--no-graph"])):
        r = subprocess.run([sys.executable, "bench.py"] + BENCH + extra, cwd=tree, capture_output=True, text=True, timeout=600, check=True)
        run[key] = last_json(r.stdout)["ms_per_step"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-us", tree], cwd=tree, capture_output=True, text=True, timeout=600, check=True)
    run.update(last_json(r.stdout))
    return run


def stats(runs):
    return {k: {"median": statistics.median(r[k] for r in runs), "min": min(r[k] for r in runs), "max": max(r[k] for r in runs)} for k in KEYS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-us", metavar="TREE", help="measure (c) on the checkout TREE and print it (what the driver starts per process)")
    ap.add_argument("--parent")
    ap.add_argument("--new")
    ap.add_argument("--parent-commit", default="")
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--out", default="profiles/fs2_plan_ab.json")
    args = ap.parse_args()
    if args.host_us:
        return host_us(os.path.abspath(args.host_us))
    trees = {"parent": os.path.abspath(args.parent), "new": os.path.abspath(args.new)}
    runs = []
    for tag in ["parent_aa", "parent_aa"] + ["parent", "new"] * args.processes:
        run = dict(tree=tag, **one_process_set(trees["new" if tag == "new" else "parent"]))
        runs.append(run)
        print(json.dumps(run), flush=True)
    out = {"what": "FastSpeech2: the commit before the kernel plan against the commit that introduces it, alternated in one session on one "
                   "MI355X, %d processes each, after an A/A pair of the parent" % args.processes,
           "parent_commit": args.parent_commit, "new_commit": "the commit that adds this file (its tree, on top of the parent)",
           "method": {"ms_per_step": "bench.py " + " ".join(BENCH) + ": the replayed hipGraph step",
                      "ms_per_step_eager": "the same with --no-graph",
                      "host_us_fwd_bwd": "host time of one eager _forward + backward_native at B = 16, L = 64 (perf_counter around the two "
                                         "calls, synchronised afterwards), median of 60 per process"},
           "runs": runs}
    for tag in ("parent_aa", "parent", "new"):
        out[tag] = stats([r for r in runs if r["tree"] == tag])
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
