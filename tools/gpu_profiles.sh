# All profile artifacts of the current tree: rocprofv3 kernel stats, PMC HBM traffic, MFMA/LDS
# counters, the per-launch HIP-event table -> $OUT/ (copy the ones to keep to profiles/).
set -o pipefail
export DSGAN_OUT=${DSGAN_OUT:-dsgan_out}   # $OUT: the scripts called below write there too
OUT=$DSGAN_OUT
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
bash tools/gpu_prof.sh || exit $?
bash tools/gpu_pmc.sh || exit $?
rm -rf $OUT/pmcf $OUT/pmcw
bash tools/gpu_mfma_pmc.sh || exit $?
timeout -k 10 200 python tools/launch_table.py > $OUT/launches_all.txt 2>&1
