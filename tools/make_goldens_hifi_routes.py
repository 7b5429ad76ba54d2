#!/usr/bin/env python3
"""Generate tests/golden/hifi_route_launches.json: the launch sequence of a HiFi-GAN generator forward (tests/hifi_routes_util.py) in
every case of its CASES, recorded on an MI355X from the commit whose behaviour is to be kept, and `stage_routes()` over the 32
settings of the route toggles for V1, V2 and V3.

Every case is recorded twice, each time on a fresh generator.  The launch logs must agree between the two runs (otherwise the tool
stops: the tree under it has no launch sequence to pin); the sha256 of the waveform is stored only where the two runs agree.

    python tools/make_goldens_hifi_routes.py --commit <hash of the recorded tree>
    python tools/make_goldens_hifi_routes.py --table-only          (no GPU: prints the route table)
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
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "hifi_route_launches.json"))
    ap.add_argument("--table-only", action="store_true", help="print the route table (host predicates only) and stop")
    args = ap.parse_args()
    from tests.hifi_routes_util import CASES, GRID, ROW_FRAMES, Recorder, route_table
    from tts_king_amd.config import default_config
    cfg = default_config()
    table = route_table(cfg)
    if args.table_only:
        print(json.dumps(table))
        return
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO).decode().strip()
    rec = Recorder(cfg)
    cases = {}
    for name in CASES:
        a, b = rec.record(name), rec.record(name)
        for key in ("routes", "short_rows", "raises", "launches"):
            if a.get(key) != b.get(key):
                sys.exit("case %r: two runs of the same tree disagree in %r" % (name, key))
        if a.get("wav_sha256") != b.get("wav_sha256"):
            print("case %r: the waveform bytes of two runs differ; no digest stored" % name)
            a["wav_sha256"] = None
        cases[name] = a
        print("%-28s %s short_rows %s: %s" % (name, a["routes"], a["short_rows"],
                                             a.get("raises") or "%d launches, sha256 %s" % (len(a["launches"]), str(a["wav_sha256"])[:12])))
    with open(args.out, "w") as f:
        f.write("{\n \"commit\": %s,\n \"row_frames\": %s,\n \"grid\": %s,\n \"route_table\": {\n" % (json.dumps(commit), json.dumps(ROW_FRAMES), json.dumps(list(GRID))))
        for i, (name, rows) in enumerate(table.items()):          # one toggle setting per line
            f.write("  %s: {\n   %s\n  }%s\n" % (json.dumps(name), ",\n   ".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in rows.items()),
                                                "," if i + 1 < len(table) else ""))
        f.write(" },\n \"cases\": {\n")
        for i, (name, r) in enumerate(cases.items()):
            f.write("  %s: {\n   \"routes\": %s,\n   \"short_rows\": %s" % (json.dumps(name), json.dumps(r["routes"]), json.dumps(r["short_rows"])))
            if "raises" in r:
                f.write(",\n   \"raises\": %s\n" % json.dumps(r["raises"]))
            else:                                                   # one launch per line: a changed launch shows as a changed line
                f.write(",\n   \"wav_sha256\": %s,\n   \"launches\": [\n    %s\n   ]\n" % (
                    json.dumps(r["wav_sha256"]), ",\n    ".join(json.dumps(e, separators=(",", ":")) for e in r["launches"])))
            f.write("  }%s\n" % ("," if i + 1 < len(cases) else ""))
        f.write(" }\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
