#!/bin/bash
# Interleaved same-box processes of scripts/turbo_stream_measure.py: Turbo and Nano streaming latency (two processes each, the
# one-shot call and both stream forms alternating inside each), then the batch-1 token step through cbx_gpt2_loop_run against the Python replay loop
# (three processes each, alternating).  Every step under its own time limit; the first failure ends the run.
#   scripts/turbo_stream_measure.sh OUT_DIR
set -u
OUT=${1:?output directory}
mkdir -p "$OUT"
cd "$(dirname "$0")/.."
run() {  # run LOG SECONDS ARGS...
    local log=$1 t=$2
    shift 2
    timeout -k 10 "$t" python scripts/turbo_stream_measure.py "$@" >> "$OUT/$log" 2>&1
    local rc=$?
    echo "rc=$rc: $*" >> "$OUT/$log"
    if [ $rc -ne 0 ]; then echo "step failed (rc=$rc): $*"; tail -20 "$OUT/$log"; exit $rc; fi
}
for i in 1 2; do
    run turbo_stream_latency.log 300 latency --model turbo --reps 5
    run turbo_stream_latency.log 300 latency --model nano --reps 5
done
for i in 1 2 3; do
    run turbo_stream_loop.log 200 loop --impl c --steps 200
    run turbo_stream_loop.log 200 loop --impl py --steps 200
done
grep -h '^{' "$OUT"/turbo_stream_*.log
