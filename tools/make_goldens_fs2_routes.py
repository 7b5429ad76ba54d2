#!/usr/bin/env python3
"""Generate tests/golden/fs2_route_launches.json: what FastSpeech2 launches in a train step, a teacher-forced eval forward and the two
inference halves (tests/fs2_routes_util.py) in every case of its CASES, the bits that come out and the weight packs the model holds,
recorded on an MI355X from the commit whose behaviour is to be kept.

Every case is recorded twice, each time on a fresh model.  The launch logs, the packs and the optimizer's item count must agree
between the two runs (otherwise the tool stops: the tree under it has nothing to pin); a digest is stored only where the two runs
agree, else null with the reason beside it.

    python tools/make_goldens_fs2_routes.py --commit <hash of the recorded tree>
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
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "fs2_route_launches.json"))
    args = ap.parse_args()
    import tests.fs2_routes_util as routes
    CASES, PASSES, Recorder = routes.CASES, routes.PASSES, routes.Recorder
    from tts_king_amd.config import default_config
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO).decode().strip()
    rec = Recorder(default_config())
    cases = {}
    for name in CASES:
        a, b = rec.record(name), rec.record(name)
        for key in ("launches", "packs", "adam_items", "repack_after_step"):
            if a[key] != b[key]:
                for p in PASSES if key == "launches" else ():
                    for i, (x, y) in enumerate(zip(a[key][p], b[key][p])):
                        if x != y:
                            print("%s launch %d: %s, then %s" % (p, i, x, y))
                sys.exit("case %r: two runs of the same tree disagree in %r" % (name, key))
        a["null_reasons"] = {}
        for key in a["sha256"]:
            if a["sha256"][key] != b["sha256"][key]:
                print("case %r: the %s bytes of two runs differ; no digest stored" % (name, key))
                a["sha256"][key] = None
                a["null_reasons"][key] = "two runs of the recorded commit itself gave different bytes"
        cases[name] = a
        print("%-28s %s launches, %d packs, Adam items %s, repack %s, grad sha256 %s" % (
            name, [len(a["launches"][p]) for p in PASSES], len(a["packs"]), a["adam_items"], a["repack_after_step"], str(a["sha256"]["grad"])[:12]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("{\n \"commit\": %s,\n \"cases\": {\n" % json.dumps(commit))
        for i, (name, r) in enumerate(cases.items()):
            f.write("  %s: {\n   \"config\": %s,\n   \"toggles\": %s,\n   \"adam_items\": %s,\n   \"repack_after_step\": %s,\n   \"sha256\": %s,\n   \"null_reasons\": %s,\n" % (
                json.dumps(name), json.dumps(CASES[name][0]), json.dumps(CASES[name][1]), json.dumps(r["adam_items"]), json.dumps(r["repack_after_step"]),
                json.dumps(r["sha256"]), json.dumps(r["null_reasons"])))
            f.write("   \"packs\": [\n    %s\n   ],\n   \"launches\": {\n" % ",\n    ".join(json.dumps(p, separators=(",", ":")) for p in r["packs"]) if r["packs"]
                    else "   \"packs\": [],\n   \"launches\": {\n")
            for j, p in enumerate(PASSES):                      # one launch per line: a changed launch shows as a changed line
                f.write("    %s: [\n     %s\n    ]%s\n" % (json.dumps(p), ",\n     ".join(json.dumps(e, separators=(",", ":")) for e in r["launches"][p]),
                                                          "," if j + 1 < len(PASSES) else ""))
            f.write("   }\n  }%s\n" % ("," if i + 1 < len(cases) else ""))
        f.write(" }\n}\n")
    with open(args.out) as f:
        json.load(f)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
