# Collects the per-round profile artefacts on the GPU box: kernel trace + the two PMC passes of one bench config, condensed by
# scripts/prof_summary.py into $OUT (default out/).  Usage: [OUT=dir] bash scripts/prof_cmd.sh <tag> [config] [extra bench args]
set -x
TAG=${1:-r03}
CFG=${2:-2}
shift; shift
EXTRA="$@"
R="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$(mkdir -p "${OUT:-$R/out}" && cd "${OUT:-$R/out}" && pwd)"
cd /tmp && export TMPDIR=/tmp
N=${TAG}_cfg${CFG}
B="python $R/bench.py --full --config $CFG --steps 1 --no-cpu-baseline --no-cv-leg --no-extra-legs"
# The kernel-trace pass of config 5 (eight host threads submitting to streams that share hardware queues) has crashed inside
# librocprofiler-sdk's queue-intercept layer (SIGSEGV at the end of a 1 MB queue ring mapping, below libhsa-runtime64, from
# whichever HIP call a fold thread happened to be in; never without the profiler attached, never in the PMC passes, which
# serialise dispatches).  A failed pass ends the script: it is not retried.
rm -rf $OUT/prof_${N}_k
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $OUT/prof_${N}_k -o k -- $B --warmup 1 $EXTRA > $OUT/${N}_bench_under_rocprof.json 2> $OUT/prof_${N}.err || exit 1
timeout -k 10 900 rocprofv3 --pmc FETCH_SIZE -d $OUT/prof_${N}_f -o f -- $B --warmup 0 $EXTRA > /dev/null 2>&1 || exit 1
timeout -k 10 900 rocprofv3 --pmc WRITE_SIZE -d $OUT/prof_${N}_w -o w -- $B --warmup 0 $EXTRA > /dev/null 2>&1 || exit 1
cd $R
python scripts/prof_summary.py $(find $OUT/prof_${N}_k -name "*results.db" | head -1) $(find $OUT/prof_${N}_f -name "*results.db" | head -1) $(find $OUT/prof_${N}_w -name "*results.db" | head -1) > $OUT/${N}_rocprof_summary.txt 2>&1
# the databases are large; only the summaries are kept
rm -rf $OUT/prof_${N}_k $OUT/prof_${N}_f $OUT/prof_${N}_w
