#!/bin/bash
# A focused GPU call: the named -m gpu test files (or node ids), then smoke() and the default
# bench line, each under its own limit.  usage: bash tools/gpu_quick.sh <tag> <pytest targets...>
set -o pipefail
tag=${1:?tag}; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/$tag
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest "$@" -m gpu -v -s --timeout 300 --timeout-method thread > $OUT/tests.log 2>&1 || { echo "tests failed"; grep -E "FAILED|Error|assert" $OUT/tests.log | head -30; tail -5 $OUT/tests.log; exit 1; }
tail -2 $OUT/tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { echo "smoke failed"; tail -20 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 600 python -u $R/bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { echo "bench failed"; tail -20 $OUT/bench.err; exit 1; }
cut -c1-600 $OUT/bench.json
echo "quick ok"
