#!/usr/bin/env python3
"""Generate tests/golden/pair_bits_digests.json: the sha256 of every output of the HiFi-GAN pair kernels and the ResBlock2 kernel over
the cases of tests/pair_bits_util.py, recorded on an MI355X from the build of the library whose bits are to be kept (TTSK_LIB_PATH
selects a build, as in tools/ab_libs.sh).

Every case runs twice; the tool stops when the two runs disagree (such a build has no bits to pin).

    TTSK_LIB_PATH=<parent build> python tools/make_goldens_pair_bits.py --commit <hash the library was built from>
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
    ap.add_argument("--commit", default=None, help="hash of the tree the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "pair_bits_digests.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO).decode().strip()
    from tests import pair_bits_util as U
    cases = {}
    for case in U.CASES:
        a, b = U.run_case(case), U.run_case(case)
        if a != b:
            sys.exit("case %s: two runs of the same build disagree in %s" % (U.case_id(case), sorted(k for k in a if a[k] != b[k])))
        cases[U.case_id(case)] = a
        print("%-24s %d digests" % (U.case_id(case), len(a)))
    with open(args.out, "w") as f:
        json.dump({"commit": commit, "library": os.path.relpath(os.environ.get("TTSK_LIB_PATH") or os.path.join(REPO, "tts_king_amd", "libttsk_hip.so"), REPO), "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
