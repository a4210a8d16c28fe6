set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
python bench.py --full > $OUT/r02n_bench.json 2> $OUT/r02n_bench.err && echo bench ok
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r02n_prof -- python3 bench.py --full --no-cpu-baseline --no-stage0 > $OUT/r02n_bench_under_rocprof.json 2> $OUT/r02n_prof.err && echo prof ok
f=$(find $OUT/r02n_prof -name "*kernel_stats.csv" | head -1); cp "$f" $OUT/r02n_bench_kernel_stats.csv; rm -rf $OUT/r02n_prof
bash scripts/pmc_passes.sh $OUT/r02n_pmc scripts/pmc_edit_steps.py 4 > $OUT/r02n_pmc_summary.json 2> $OUT/r02n_pmc.err && echo pmc ok
find $OUT/r02n_pmc -name "*.csv" -delete; find $OUT/r02n_pmc -type d -empty -delete
