#!/bin/bash
# SQ counters of the headline's gm_rollout launches: rocprofv3 --pmc, two passes (sq1, sq2),
# each a run of its own with no tracing beside it, over the bench headline alone (--steps 10
# --warmup 10: two 10-env-step rollout launches after the per-step pre-roll), then
# tools/pmc_sq_rollout_summary.py.  usage (on a machine with the GPU):
#   bash tools/pmc_sq_rollout.sh <output directory> [out.json]
set -o pipefail
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
[ -n "$1" ] || { echo "usage: bash tools/pmc_sq_rollout.sh <output directory> [out.json]"; exit 2; }
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
JSON=${2:-$OUT/pmc_sq.json}
case $JSON in /*) ;; *) JSON=$(pwd)/$JSON ;; esac
HL="python3 $R/bench.py --full --steps 10 --warmup 10 --no-cpu --no-parity --no-policy --no-c2 --no-random --no-scripted --no-c1"
cd /tmp && export TMPDIR=/tmp
pass() { local name=$1; shift; timeout -k 10 240 rocprofv3 --pmc "$@" --output-format csv -d $OUT/$name -o run -- $HL > $OUT/$name.log 2>&1 || { echo "pass $name failed"; tail -5 $OUT/$name.log; exit 1; }; echo "pass $name ok"; }
pass sq1 SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVES
pass sq2 SQ_INSTS_SALU SQ_INSTS_SMEM SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_THREAD_CYCLES_VALU
python3 $R/tools/pmc_sq_rollout_summary.py $OUT 10 4096 $JSON > /dev/null && echo "summary ok"
