# rocprofv3 kernel-trace stats of one bench step (env passed through, e.g. VLOG_AMD_XSPLITS=1); TAG names the output,
# OUT the folder it goes to (default bench_out/ in the repository)
set -o pipefail
R=${REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${OUT:-$R/bench_out}
mkdir -p $OUT
TAG=${TAG:-prof}
cd /tmp && export TMPDIR=/tmp
# --full: the trace also covers the bench's event-profiled step, its parity step and its variable block
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python3 $R/bench.py --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1 || { tail -20 $OUT/prof_$TAG.log; exit 1; }
F=$(ls $OUT/prof_$TAG/*kernel_stats.csv | head -1)
python3 - "$F" <<'PY'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
for r in rows[:22]:
    print(f"{float(r['TotalDurationNs'])/3e6:9.1f} ms/step {int(r['Calls'])//3:7d} calls/step {float(r['AverageNs'])/1e3:9.2f} us  {r['Name'][:90]}")
PY
