# Round GPU check: smoke, the GPU test suite, a short bench.  Each step under
# its own time limit; stop at the first failure.
RES=${RES:-out}  # results directory
set -u
mkdir -p $RES
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $RES/smoke.log 2>&1; rc=$?; echo smoke=$rc
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v -p no:cacheprovider --timeout 120 --timeout-method thread > $RES/gputests.log 2>&1; rc=$?; echo tests=$rc
if [ $rc -ne 0 ]; then tail -30 $RES/gputests.log; exit $rc; fi
timeout -k 10 400 python bench.py --full --steps 100 --warmup 10 > $RES/bench.log 2>&1; echo bench=$?
