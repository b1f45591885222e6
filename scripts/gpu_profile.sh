#!/bin/bash
# The round profile: all GPU tests, smoke, the default bench, the same bench
# under rocprofv3 --kernel-trace --stats, bench_rows.py, the FETCH_SIZE /
# WRITE_SIZE PMC passes of the C2 bench (sections c2, from_traces, steady) and
# of the C3 two-phase per-rank step (section c3), their summary into
# profiles/pmc_traffic.json of this copy, the default bench again (reading
# it), and the N=2 gloo rehearsal through bench.py's own launcher.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
T=${TAG:-r05}
if [ -z "$NOTEST" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread > $OUT/pytest_gpu_$T.log 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -2 $OUT/pytest_gpu_$T.log
  [ $rc -eq 0 ] || exit $rc
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$T.log 2>&1
  rc=$?; echo "smoke rc=$rc"; [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$T -o run --output-format csv -- python3 bench.py --full --no-cpu > $OUT/prof_bench_$T.log 2>&1
rc=$?; echo "rocprof stats rc=$rc"; [ $rc -eq 0 ] || exit $rc
if [ -z "$NOROWS" ]; then
  timeout -k 10 900 python -u bench_rows.py > $OUT/rows_$T.jsonl 2> $OUT/rows_$T.err
  rc=$?; echo "rows rc=$rc"; [ $rc -eq 0 ] || exit $rc
fi
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 -s KILL 300 rocprofv3 --pmc $C -d $OUT/pmc_${C}_$T -o run --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu --no-account > $OUT/pmc_${C}_$T.log 2>&1
  rc=$?; echo "pmc $C rc=$rc"; [ $rc -eq 0 ] || exit $rc
  timeout -k 10 -s KILL 300 rocprofv3 --pmc $C -d $OUT/pmc_${C}_${T}c3 -o run --output-format csv -- python3 bench.py --full --mode c3 --c3-two-phase --steps 2 --warmup 1 --no-cpu --no-account > $OUT/pmc_${C}_${T}c3.log 2>&1
  rc=$?; echo "pmc c3 $C rc=$rc"; [ $rc -eq 0 ] || exit $rc
done
F=$(find $OUT/pmc_FETCH_SIZE_$T -name '*counter_collection.csv' | head -1)
W=$(find $OUT/pmc_WRITE_SIZE_$T -name '*counter_collection.csv' | head -1)
python3 scripts/pmc_summary.py "$F" "$W" $OUT/pmc_traffic.json $T > $OUT/pmcsum_$T.log 2>&1 || exit 1
F=$(find $OUT/pmc_FETCH_SIZE_${T}c3 -name '*counter_collection.csv' | head -1)
W=$(find $OUT/pmc_WRITE_SIZE_${T}c3 -name '*counter_collection.csv' | head -1)
python3 scripts/pmc_summary.py "$F" "$W" $OUT/pmc_traffic.json ${T}c3 c3 merge >> $OUT/pmcsum_$T.log 2>&1 || exit 1
cp $OUT/pmc_traffic.json profiles/pmc_traffic.json
echo "pmc summary done"
timeout -k 10 600 python -u bench.py --full --pipeline > $OUT/bench_$T.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -1 $OUT/bench_$T.log | cut -c1-300
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -u bench.py --full --mode c3 --c3-two-phase > $OUT/bench_c3_$T.log 2>&1
rc=$?; echo "bench c3 rc=$rc"; tail -1 $OUT/bench_c3_$T.log | cut -c1-300
[ $rc -eq 0 ] || exit $rc
SG_BENCH_BACKEND=gloo timeout -k 10 600 python3 bench.py --full --gpus 2 --programs 16384 > $OUT/gloo2_$T.log 2>&1
rc=$?; echo "gloo2 rc=$rc"; tail -1 $OUT/gloo2_$T.log | cut -c1-300
exit $rc
