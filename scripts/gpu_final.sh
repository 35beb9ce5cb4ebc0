# Full check of the tree on a fresh box: every GPU test, smoke, a kernel-trace profile of the
# bench, the full bench line, and the HBM traffic (FETCH_SIZE / WRITE_SIZE passes) of the default
# C3 backward. Usage: TAG=r4k STAGE=tests|bench [OUT=dir] bash scripts/gpu_final.sh (two calls:
# each stays within one session's time limit)
set -o pipefail
TAG=${TAG:-r4k}
STAGE=${STAGE:-tests}
OUT=${OUT:-check_out}
mkdir -p $OUT
export TMPDIR=/tmp
export MT_PARITY_OUT=$OUT/parity.json
if [ "$STAGE" = tests ]; then
timeout -k 10 1080 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread -p no:cacheprovider > $OUT/tests_$TAG.log 2>&1
rc=$?; tail -3 $OUT/tests_$TAG.log; grep -E "FAILED|ERROR" $OUT/tests_$TAG.log | head; [ $rc -eq 0 ] || exit $rc
cp $OUT/parity.json $OUT/parity_$TAG.json 2>/dev/null
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1; rc=$?; tail -2 $OUT/smoke_$TAG.log; [ $rc -eq 0 ] || exit $rc
exit 0
fi
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py --steps 100 --warmup 20 --full --no-cpu > $OUT/prof_$TAG.log 2>&1; rc=$?; echo prof rc=$rc; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err; rc=$?; cat $OUT/bench_$TAG.json; [ $rc -eq 0 ] || exit $rc
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 -s KILL 240 rocprofv3 --pmc $c --kernel-trace --kernel-include-regex "fa_bwd" -d $OUT/pmcbwd_${TAG}_$c -o run --output-format csv -- python3 scripts/ablate_bwd.py 0 > $OUT/pmcbwd_${TAG}_$c.log 2>&1 || { echo "pmc $c failed"; exit 1; }
done
echo pmc ok
