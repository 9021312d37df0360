# GPU tests + bench A/B on an env knob (one call); every GPU step time-limited, chained with &&.  OUT: the folder the
# logs and lines go to (default bench_out/ in the repository)
set -o pipefail
R=${REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd $R
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
TAG=${TAG:-ab}
KNOB=${KNOB:-VLOG_AMD_DEC_SPLIT=0}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/gpu_tests_$TAG.log 2>&1 && tail -3 $OUT/gpu_tests_$TAG.log &&
timeout -k 10 600 python bench.py --full --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err && cat $OUT/bench_$TAG.json &&
env $KNOB timeout -k 10 600 python bench.py --full --no-cpu-baseline > $OUT/bench_${TAG}_b.json 2> $OUT/bench_${TAG}_b.err && cat $OUT/bench_${TAG}_b.json
rc=$?
[ $rc -ne 0 ] && tail -30 $OUT/gpu_tests_$TAG.log $OUT/bench_$TAG.err $OUT/bench_${TAG}_b.err 2>/dev/null
exit $rc
