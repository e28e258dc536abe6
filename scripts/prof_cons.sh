# kernel trace of the constrained-groups path (device visits only); writes $OUT/<tag>_cons_rocprof_summary.txt (default out/)
# Usage: [OUT=dir] bash scripts/prof_cons.sh <tag>
TAG=${1:-r05}
R="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$(mkdir -p "${OUT:-$R/out}" && cd "${OUT:-$R/out}" && pwd)"
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_cons_k
BENCH_CONS_DEVICE_ONLY=1 timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_cons_k -o k -- python $R/scripts/bench_cons.py 100000 10000 10 200 50 > $OUT/${TAG}_cons_bench_under_rocprof.json 2> $OUT/prof_cons.err || exit 1
cd $R
python scripts/prof_summary.py $(find $OUT/prof_cons_k -name "*results.db" | head -1) > $OUT/${TAG}_cons_rocprof_summary.txt 2>&1
rm -rf $OUT/prof_cons_k
head -24 $OUT/${TAG}_cons_rocprof_summary.txt
