set -o pipefail
OUT=${DSGAN_OUT:-dsgan_out}   # results: the directory $DSGAN_OUT names, dsgan_out/ by default
mkdir -p "$OUT"
for d in 1 0 1 0; do
  DSGAN_DEFER_SPLITS=$d timeout -k 10 300 python -u bench.py --steps 20 --warmup 5 > "$OUT/ab_$d.log" 2>&1 || exit 1
  echo "defer=$d $(tail -1 "$OUT/ab_$d.log" | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["ms_per_step"])')"
done
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-quality --no-train-equiv > "$OUT/prof.log" 2>&1 || exit 1
python3 tools/prof_stats.py "$OUT/prof/run_results.db" "$OUT/prof_stats.csv" --steps 15 > "$OUT/prof_top.txt" 2>&1
python3 tools/prof_dispatch.py "$OUT/prof/run_results.db" "$OUT/prof_dispatch.csv" --last 786 || true
rm -rf "$OUT/prof"
