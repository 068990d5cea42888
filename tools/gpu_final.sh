#!/bin/bash
# Round-end evidence on the GPU box, in the driver's order: GPU tests, smoke(), the default bench
# line (every leg), then the headline's rocprofv3 kernel stats + FETCH/WRITE passes.
#   tools/gpu_final.sh TAG     -> $OUT/<TAG>_pytest.log, <TAG>_smoke.log, <TAG>_bench.json (OUT: bench_out),
#                                 the profiles where tools/gpu_profile.sh puts them
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
TAG=${1:-final}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export PYTHONUNBUFFERED=1
timeout -k 10 700 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread \
    > $OUT/${TAG}_pytest.log 2>&1
rc=$?; tail -n 3 $OUT/${TAG}_pytest.log
[ $rc -le 1 ] || { echo "pytest exit $rc"; exit $rc; }
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 \
    || { tail -n 5 $OUT/${TAG}_smoke.log; exit 1; }
tail -n 1 $OUT/${TAG}_smoke.log
timeout -k 10 600 python -u bench.py --full --detail "$OUT/${TAG}_bench_detail.json" > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err \
    || { tail -n 5 $OUT/${TAG}_bench.err; exit 1; }
tail -c 400 $OUT/${TAG}_bench.json
WORKLOADS="b128_easy|" timeout -k 10 400 bash tools/gpu_profile.sh
