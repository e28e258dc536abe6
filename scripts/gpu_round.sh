# One GPU-box visit: the -m gpu suite, then one full bench line per BASELINE.json config (with CPU baselines); stops at the
# first failing step.  Results go to $OUT (default out/).
# Usage: [OUT=dir] bash scripts/gpu_round.sh <tag> "<pytest -k expression or empty>" [configs...]
TAG=${1:-r02}; KEXPR=${2:-}; shift; shift
CFGS=${@:-"2 3 5 4"}
OUT=${OUT:-out}
mkdir -p $OUT
if [ -n "$KEXPR" ]; then
  timeout -k 10 1500 python -m pytest tests -m gpu -x -q -k "$KEXPR" > $OUT/${TAG}_pytest.log 2>&1
else
  timeout -k 10 1500 python -m pytest tests -m gpu -x -q > $OUT/${TAG}_pytest.log 2>&1
fi
rc=$?; echo "pytest rc=$rc" | tee -a $OUT/${TAG}_pytest.log
tail -5 $OUT/${TAG}_pytest.log
[ $rc -eq 0 ] || exit $rc
for c in $CFGS; do
  [ "$c" = "none" ] && break
  timeout -k 10 900 python bench.py --full --config $c > $OUT/${TAG}_cfg$c.json 2> $OUT/${TAG}_cfg$c.err
  rc=$?; echo "cfg $c rc=$rc"
  tail -c 600 $OUT/${TAG}_cfg$c.err | tail -3
  cut -c1-900 $OUT/${TAG}_cfg$c.json
  [ $rc -eq 0 ] || exit $rc
done
