#!/bin/bash
# On an MI355X: GPU tests, smoke, the bench line, and a rocprofv3 kernel trace of a --full bench run.  Output -> $OUT (default: a
# directory under the temp directory).  A step that faults, aborts or runs out of time ends the script: nothing more is started.
# usage: [OUT=dir] bash tools/gpu_check.sh [pytest-args...]   (default: the whole -m gpu suite)
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT:-${TMPDIR:-/tmp}/ttsk_gpu_check}
mkdir -p $O
cd $R
export TMPDIR=/tmp
gate() { case $1 in 124|134|137|139) echo "stopping after rc=$1"; exit $1;; esac; }
ARGS=${@:-tests}
timeout -k 10 900 python -m pytest $ARGS -m gpu -q -s > $O/pytest_gpu.log 2>&1; rc=$?; echo "pytest rc=$rc" | tee -a $O/pytest_gpu.log
grep -E "rel-RMS|passed|failed|Error|error" $O/pytest_gpu.log | tail -40; gate $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; rc=$?; echo "smoke rc=$rc" | tee -a $O/smoke.log
tail -2 $O/smoke.log; gate $rc
timeout -k 10 600 python bench.py > $O/bench.json 2> $O/bench.err; rc=$?; echo "bench rc=$rc"
tail -c 4000 $O/bench.json; gate $rc
# the interpreter itself, not a launcher script, goes after rocprofv3's --
PY=$(python -c "import sys; print(sys.executable)")
cd /tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o fs2 -- "$PY" $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-roofline --no-mel --no-e2e > $O/prof_bench.log 2>&1; echo "rocprof rc=$?"
find $O/prof -name "*stats*" | head
