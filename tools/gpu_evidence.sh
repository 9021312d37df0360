# Round evidence in one call, every GPU step under its own time limit and chained with &&:
#   1. the GPU suite as the driver runs it (python -m pytest tests -m gpu), log under $OUT (default bench_out/)
#   2. the driver's bench command with every block (python3 bench.py --gpus 1 --steps 20 --warmup 5 --full), with its wall time
#   3. rocprofv3 --kernel-trace --stats of a short bench run (same kernels)
#   4. PMC HBM-traffic passes of the dominant kernel (tools/pmc_traffic.sh)
# SKIP_TESTS=1 / SKIP_BENCH=1 / SKIP_PROF=1 / NO_PMC=1 drop steps; WORKER=1 appends the worker-call lines
# (tools/bench_worker_call.py: margin model, and random weights at T=0 as round 2 measured).  TAG names the outputs.
set -o pipefail
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/bench_out}
cd $R && mkdir -p $OUT
TAG=${TAG:-r03}
export VLOG_AMD_PROGRESS=$OUT/progress_$TAG.log
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --durations=20 --timeout 600 --timeout-method thread > $OUT/gpu_tests_$TAG.log 2>&1
  rc=$?; tail -3 $OUT/gpu_tests_$TAG.log
  [ $rc -ne 0 ] && { grep -E "FAILED|Error|assert" $OUT/gpu_tests_$TAG.log | head -30; exit $rc; }
fi
[ -n "$SKIP_BENCH" ] && exit 0
t0=$(date +%s.%N)
timeout -k 10 900 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -30 $OUT/bench_$TAG.err; exit 1; }
t1=$(date +%s.%N)
echo "{\"cmd\": \"python3 bench.py --gpus 1 --steps 20 --warmup 5 --full\", \"wall_s\": $(python3 -c "print(round($t1-$t0,1))")}" > $OUT/bench_${TAG}_wall.json
cat $OUT/bench_$TAG.json $OUT/bench_${TAG}_wall.json
[ -n "$SKIP_PROF" ] && exit 0
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python3 $R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-parity --no-variable > $OUT/prof_$TAG.log 2>&1 || { tail -30 $OUT/prof_$TAG.log; exit 1; }
head -25 $(ls $OUT/prof_$TAG/*kernel_stats.csv | head -1) | cut -d, -f1-5
tail -1 $OUT/prof_$TAG.log
if [ -z "$NO_PMC" ]; then
  BENCH_ARGS=--no-variable bash $R/tools/pmc_traffic.sh || exit 1
fi
[ -z "$WORKER" ] && exit 0
cd $R
timeout -k 10 600 python tools/bench_worker_call.py --minutes-seq 2 --minutes-tp 30 > $OUT/worker_$TAG.json 2> $OUT/worker_$TAG.err || { tail -20 $OUT/worker_$TAG.err; exit 1; }
cat $OUT/worker_$TAG.json
timeout -k 10 600 python tools/bench_worker_call.py --minutes-seq 2 --minutes-tp 30 --random-weights --temperature 0 > $OUT/worker_${TAG}_random_t0.json 2> $OUT/worker_${TAG}_random_t0.err || { tail -20 $OUT/worker_${TAG}_random_t0.err; exit 1; }
cat $OUT/worker_${TAG}_random_t0.json
