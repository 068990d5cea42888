#!/bin/bash
# A/B of the f-only pack kernels: multi-row LDS tiles (FMPNP_PACK_F_ROWS=1) vs LDS tiles (=0)
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-bench_out}  # logs, lines and detail files
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest tests/test_window_pack.py tests/test_layout_f.py tests/test_batch_prep.py -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/packreg_tests.log 2>&1 || { tail -30 $OUT/packreg_tests.log; exit 1; }
tail -2 $OUT/packreg_tests.log
for rep in 1 2; do
  for reg in 0 1; do
    FMPNP_PACK_F_ROWS=$reg timeout -k 10 200 python bench.py --full --legs pack,pipeline --steps 200 --warmup 5 --detail $OUT/packab_${reg}_${rep}.json > $OUT/packab_${reg}_${rep}.line 2> $OUT/packab_${reg}_${rep}.err || { tail $OUT/packab_${reg}_${rep}.err; exit 1; }
    python - "$reg" "$rep" "$OUT/packab_${reg}_${rep}.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[3]))
e = d["end_to_end"]
print(f"rows={sys.argv[1]} rep={sys.argv[2]} pack_f {d['pack_f']['ms']} ms {d['pack_f']['frac_of_peak']}  e2e {e['queries_per_s']} q/s steady {e['steady_state_queries_per_s']} hard {e['hard_init']['queries_per_s']} full {e['full_pack']['queries_per_s']} same {e['identical_to_full_pack']} robotcar {e['robotcar_1664'].get('queries_per_s')}")
PY
  done
done
