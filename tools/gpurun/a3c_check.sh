#!/bin/bash
# GPU job: A3C GPU tests, config-3 train-step traces (a3c_prof.sh) and the bench line with extras.
set -o pipefail
O=${1:-build/a3c_check}   # usage: a3c_check.sh [output folder]
mkdir -p $O && timeout -k 10 400 python -u -m pytest tests/test_a3c_gpu.py -x -q --timeout 120 --timeout-method thread > $O/pytest_a3c.log 2>&1; rc=$?; tail -3 $O/pytest_a3c.log; [ $rc -eq 0 ] && bash $(dirname $0)/a3c_prof.sh && timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_a3c.json 2> $O/bench_a3c.err && python tools/show_extras.py $O/bench_a3c.json
