#!/usr/bin/env python3
"""Generate tests/golden/dw_schedule_launches.json: the launch sequence of the FastSpeech2 backward's deferred weight-gradient work
(tests/dw_schedule_util.py) in seven configurations, recorded on an MI355X from the commit whose behaviour is to be kept.

Every configuration is recorded twice.  The launch log, the launch counts and the trace must agree between the two runs (otherwise
the tool stops: the tree under it has no launch sequence to pin); the sha256 of the gradient buffer is stored only where they agree.

    python tools/make_goldens_dw_schedule.py --commit <hash of the recorded tree>
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="hash of the recorded tree (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "dw_schedule_launches.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO).decode().strip()
    from tests.dw_schedule_util import BUCKET_MB, CONFIGS, Recorder
    from tts_king_amd.config import default_config
    rec = Recorder(default_config())
    out = {"commit": commit, "bucket_mb": BUCKET_MB, "configs": {}}
    for name in CONFIGS:
        a, b = rec.record(name), rec.record(name)
        for key in ("launches", "counts", "trace"):
            if a[key] != b[key]:
                if key != "counts":
                    i = next((i for i, (x, y) in enumerate(zip(a[key], b[key])) if x != y), min(len(a[key]), len(b[key])))
                    print("%s: %d / %d entries, first difference at %d:\n  %s\n  %s" % (key, len(a[key]), len(b[key]), i, a[key][i:i + 4], b[key][i:i + 4]))
                sys.exit("configuration %r: two runs of the same tree disagree in %r" % (name, key))
        if a["grad_sha256"] != b["grad_sha256"]:
            print("configuration %r: the gradient bytes of two runs differ; no digest stored" % name)
            a["grad_sha256"] = None
        out["configs"][name] = a
        print("%-22s %4d launches, %d buckets, %d streams, trace %d, counts %s" % (
            name, len(a["launches"]), sum(e[0] == "bucket" for e in a["launches"]), 1 + max(e[-1 if e[0] == "bucket" else 1] for e in a["launches"]),
            len(a["trace"]), a["counts"]))
    with open(args.out, "w") as f:
        f.write("{\n \"commit\": %s,\n \"bucket_mb\": %d,\n \"configs\": {\n" % (json.dumps(commit), BUCKET_MB))
        for i, (name, r) in enumerate(out["configs"].items()):
            f.write("  %s: {\n" % json.dumps(name))
            f.write("   \"grad_sha256\": %s,\n   \"counts\": %s,\n" % (json.dumps(r["grad_sha256"]), json.dumps(r["counts"])))
            for key in ("launches", "trace"):          # one entry per line: a changed launch shows as a changed line
                f.write("   %s: [\n    %s\n   ]%s\n" % (json.dumps(key), ",\n    ".join(json.dumps(e, separators=(",", ":")) for e in r[key]),
                                                         "," if key == "launches" else ""))
            f.write("  }%s\n" % ("," if i + 1 < len(out["configs"]) else ""))
        f.write(" }\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
