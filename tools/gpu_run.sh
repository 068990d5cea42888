#!/bin/bash
# One GPU session: GPU tests (optionally a subset), then a headline bench (LEGS: the legs beside it).
#   tools/gpu_run.sh TAG [PYTEST_ARGS...]
# Logs: $OUT/<TAG>_pytest.log, $OUT/<TAG>_bench.json / .err (OUT: bench_out).
# A test run that crashed (exit status other than 0/1: fault, abort, timeout) ends the call.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
TAG=${1:-run}; shift
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export PYTHONUNBUFFERED=1
if [ "${SKIP_TESTS:-0}" != 1 ]; then
  timeout -k 10 ${TEST_TIMEOUT:-900} python -u -m pytest tests -m gpu -v --maxfail=${MAXFAIL:-20} \
      --timeout 300 --timeout-method thread "$@" > $OUT/${TAG}_pytest.log 2>&1
  rc=$?
  tail -n 40 $OUT/${TAG}_pytest.log
  if [ $rc -gt 1 ]; then echo "pytest exit $rc: stopping"; exit $rc; fi
fi
if [ "${SKIP_BENCH:-0}" != 1 ]; then
  timeout -k 10 ${BENCH_TIMEOUT:-300} python -u bench.py --steps ${STEPS:-2000} --full --legs ${LEGS:-none} --detail "$OUT/${TAG}_bench_detail.json" \
      > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
  rc=$?
  tail -c 3000 $OUT/${TAG}_bench.json; tail -n 5 $OUT/${TAG}_bench.err
  exit $rc
fi
