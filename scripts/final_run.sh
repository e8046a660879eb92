#!/bin/bash
# Round-end measurement set (one GPU session): the full bench line + rocprofv3 kernel stats of the same command.
# (PMC passes: scripts/pmc_run.sh -- separate runs, rocprofv3 --pmc does not survive hipGraph replays.)
#     scripts/final_run.sh OUT_DIR
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${1:?usage: scripts/final_run.sh OUT_DIR}" && cd "$1" && pwd)
cd $R
CBX_BENCH_VERBOSE=1 timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err
tail -1 $O/bench.json | cut -c1-400
cd /tmp && export TMPDIR=/tmp
timeout 700 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_bench -o bench -- python $R/bench.py --full > $O/bench_under_rocprof.json 2> /tmp/rocprof_bench.err
cp $(find /tmp/prof_bench -name "*kernel_stats.csv" | head -1) $O/bench_kernel_stats.csv
head -14 $O/bench_kernel_stats.csv | cut -c1-150
