# rocprofv3 kernel stats of a short bench run (no CPU legs), summarised on the box -> $OUT/prof_stats.csv
# ($OUT: the directory $DSGAN_OUT names, dsgan_out/ under the repository root by default)
set -o pipefail
OUT=${DSGAN_OUT:-dsgan_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-quality --no-train-equiv > "$OUT/prof.log" 2>&1; rc=$?
tail -1 "$OUT/prof.log" | cut -c1-300
# 15 executed steps: bench.py --full with HIP graphs runs 1 eager warm step, 2 warmup replays, 10 timed replays and
# 2 eager steps that time the roofline leg (bench.EAGER_TIMING_STEPS)
python3 tools/prof_stats.py "$OUT/prof/run_results.db" "$OUT/prof_stats.csv" --steps 15 > "$OUT/prof_top.txt" 2>&1
python3 tools/prof_dispatch.py "$OUT/prof/run_results.db" "$OUT/prof_dispatch.csv" --last 786 || true
cp "$OUT/prof/run_kernel_stats.csv" "$OUT/prof_kernel_stats.csv" 2>/dev/null
rm -rf "$OUT/prof"
exit $rc
