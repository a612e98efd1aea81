# HBM traffic per kernel family: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) over a short bench.
# Results under $OUT: the directory $DSGAN_OUT names, dsgan_out/ under the repository root by default.
set -o pipefail
OUT=${DSGAN_OUT:-dsgan_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
B="python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-quality --no-train-equiv"
timeout -s KILL 240 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d "$OUT/pmcf" -o run -- $B > "$OUT/pmcf.log" 2>&1 &&
timeout -s KILL 240 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d "$OUT/pmcw" -o run -- $B > "$OUT/pmcw.log" 2>&1 &&
python3 tools/pmc_traffic.py "$OUT/pmcf/run_results.db" "$OUT/pmcw/run_results.db" "$OUT/pmc_traffic.json"
