# round-3 measurement set: bench line, rocprofv3 kernel stats of the same command, counter passes of the edit's kernels and of the
# forward GEMM alone.  usage (on the GPU box): bash scripts/round3_measure.sh <tag>
set -o pipefail
tag=${1:-r03_a}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
python bench.py --full > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err && echo bench ok
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_prof -- python3 bench.py --full --no-cpu-baseline --no-stage0 --no-variants --no-gemm-ab > $OUT/${tag}_bench_under_rocprof.json 2> $OUT/${tag}_prof.err && echo prof ok
f=$(find $OUT/${tag}_prof -name "*kernel_stats.csv" | head -1); cp "$f" $OUT/${tag}_bench_kernel_stats.csv; rm -rf $OUT/${tag}_prof
bash scripts/pmc_passes.sh $OUT/${tag}_pmc_lin scripts/pmc_linear.py > $OUT/${tag}_pmc_linear_summary.json 2> $OUT/${tag}_pmc_lin.err && echo pmc linear ok
find $OUT/${tag}_pmc_lin -name "*.csv" -delete; find $OUT/${tag}_pmc_lin -type d -empty -delete
bash scripts/pmc_passes.sh $OUT/${tag}_pmc scripts/pmc_edit_steps.py 4 > $OUT/${tag}_pmc_edit_summary.json 2> $OUT/${tag}_pmc.err && echo pmc edit ok
find $OUT/${tag}_pmc -name "*.csv" -delete; find $OUT/${tag}_pmc -type d -empty -delete
