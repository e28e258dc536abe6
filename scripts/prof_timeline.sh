# idle-gap analysis of one config's kernel trace: $OUT/<tag>_cfg<c>_timeline.txt (default out/)
# Usage: [OUT=dir] bash scripts/prof_timeline.sh <tag> [config]
TAG=${1:-r05}; CFG=${2:-2}
R="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$(mkdir -p "${OUT:-$R/out}" && cd "${OUT:-$R/out}" && pwd)"
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_tl
timeout -k 10 900 rocprofv3 --kernel-trace -d $OUT/prof_tl -o k -- python $R/bench.py --full --config $CFG --steps 2 --warmup 1 --no-cpu-baseline --no-cv-leg --no-extra-legs > /dev/null 2> $OUT/prof_tl.err || exit 1
cd $R
python scripts/timeline.py $(find $OUT/prof_tl -name "*results.db" | head -1) --top 22 > $OUT/${TAG}_cfg${CFG}_timeline.txt 2>&1
rm -rf $OUT/prof_tl
cat $OUT/${TAG}_cfg${CFG}_timeline.txt
