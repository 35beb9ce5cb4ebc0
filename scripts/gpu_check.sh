# GPU session: parity tests, smoke, kernel-trace profile of the bench, full bench line.
# Usage (from the repo root on the GPU box): [OUT=dir] bash scripts/gpu_check.sh [TAG]
set -o pipefail
TAG=${1:-r1}
OUT=${OUT:-check_out}
mkdir -p $OUT
export TMPDIR=/tmp
export MT_PARITY_OUT=$OUT/parity.json
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT/tests_$TAG.log 2>&1 \
  && timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 \
  && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv \
       -- python3 bench.py --steps 100 --warmup 20 --full --no-cpu > $OUT/prof_$TAG.log 2>&1 \
  && timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
rc=$?
tail -3 $OUT/tests_$TAG.log
cat $OUT/smoke_$TAG.log $OUT/bench_$TAG.json 2>/dev/null
exit $rc
