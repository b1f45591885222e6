#!/bin/bash
# One GPU iteration, each step under its own time limit, stopping at the first
# failure: pytest ($PYTEST_ARGS, default all -m gpu tests; NOTEST=1 skips), the
# bench ($BENCH_ARGS; NOBENCH=1 skips), an optional second bench ($BENCH2 =
# bench.py args), optional bench_rows.py rows ($ROWS = its args, e.g. "c5 f4"),
# and an optional rocprofv3 kernel trace of a short bench (PROF=1).  TAG names
# the outputs under $OUT/.  The parameterised runner for every
# iteration (the round profile is gpu_profile.sh).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
TAG=${TAG:-iter}
if [ -z "$NOTEST" ]; then
  timeout -k 10 ${TEST_LIMIT:-900} python -u -m pytest ${PYTEST_ARGS:-tests -m gpu} -x -v -p no:cacheprovider \
    --timeout 300 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1
  rc=$?; echo "pytest rc=$rc"; grep -E "passed|failed|error" $OUT/pytest_$TAG.log | tail -3
  [ $rc -eq 0 ] || exit $rc
fi
if [ -z "$NOBENCH" ]; then
  timeout -k 10 600 python -u bench.py --full ${BENCH_ARGS:-} > $OUT/bench_$TAG.log 2>&1
  rc=$?; echo "bench rc=$rc"; tail -1 $OUT/bench_$TAG.log | cut -c1-400
  [ $rc -eq 0 ] || exit $rc
fi
if [ -n "$BENCH2" ]; then
  timeout -k 10 600 python -u bench.py $BENCH2 > $OUT/bench2_$TAG.log 2>&1
  rc=$?; echo "bench2 rc=$rc"; tail -1 $OUT/bench2_$TAG.log | cut -c1-400
  [ $rc -eq 0 ] || exit $rc
fi
if [ -n "$ROWS" ]; then
  timeout -k 10 900 python -u bench_rows.py $ROWS > $OUT/rows_$TAG.jsonl 2> $OUT/rows_$TAG.err
  rc=$?; echo "rows rc=$rc"; grep -c row $OUT/rows_$TAG.jsonl
  [ $rc -eq 0 ] || exit $rc
fi
if [ -n "$PROF" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- \
    python3 bench.py --full --steps 4 --warmup 1 --no-cpu --no-account --no-steady > $OUT/prof_$TAG.log 2>&1
  rc=$?; echo "rocprof rc=$rc"
  [ $rc -eq 0 ] || exit $rc
fi
exit 0
