# End-of-round artefacts: full -m gpu suite, the default bench line, one bench line per config (--full: with CPU baselines and
# the parity fields), rocprof summaries (kernel trace + PMC passes per config, constrained path).  Stops at the first failing
# step.  Results go to $OUT (default out/).  Usage: [OUT=dir] bash scripts/gpu_final.sh <tag>
TAG=${1:-r05}
export OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 1800 python -m pytest tests -m gpu -q > $OUT/${TAG}_gpu_pytest.log 2>&1
rc=$?; echo "pytest rc=$rc" | tee -a $OUT/${TAG}_gpu_pytest.log
tail -3 $OUT/${TAG}_gpu_pytest.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 1200 python bench.py --full > $OUT/${TAG}_default_line.json 2> $OUT/${TAG}_default_line.err
rc=$?; echo "default line rc=$rc"
cut -c1-200 $OUT/${TAG}_default_line.json
[ $rc -eq 0 ] || exit $rc
for c in 2 3 5 4; do
  timeout -k 10 1200 python bench.py --full --config $c > $OUT/${TAG}_cfg${c}_bench.json 2> $OUT/${TAG}_cfg${c}_bench.err
  rc=$?; echo "cfg $c rc=$rc"
  cut -c1-200 $OUT/${TAG}_cfg${c}_bench.json
  [ $rc -eq 0 ] || exit $rc
done
for c in 2 3 5 4; do bash scripts/prof_cmd.sh ${TAG} $c > $OUT/prof_${TAG}_cfg$c.log 2>&1 || exit 1; done
bash scripts/prof_cons.sh ${TAG} > /dev/null 2>&1 || exit 1
ls $OUT | grep ${TAG} | head -40
