# default bench line (with cpu_baseline) + kernel-trace stats of the same command
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u bench.py --full > $OUT/bench_default.log 2>&1 || exit 1
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o p -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/bench_prof.log 2>&1 || exit 2
