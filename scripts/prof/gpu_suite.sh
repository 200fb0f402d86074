set -o pipefail
# full GPU check: smoke, the benchmark with its secondary numbers, the GPU tests; logs go to $OUT
OUT=${OUT:-suite_out}
mkdir -p "$OUT"
timeout -k 10 120 python -u __graft_entry__.py smoke > "$OUT/smoke.log" 2>&1 || { tail -20 "$OUT/smoke.log"; exit 1; }
tail -1 "$OUT/smoke.log"
S0=$SECONDS; timeout -k 10 300 python bench.py --full > "$OUT/bench1.json" 2>"$OUT/bench1.err" || { tail -20 "$OUT/bench1.err"; exit 1; }
cat "$OUT/bench1.json"; echo "bench_wall_s $((SECONDS - S0))"
timeout -k 10 1000 python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread -p no:cacheprovider -rf > "$OUT/gputests.log" 2>&1
rc=$?
tail -15 "$OUT/gputests.log"
exit $rc
