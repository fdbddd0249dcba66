#!/bin/bash
# One GPU-box session: parity tests, then (only if the tests did not crash)
# the bench and a rocprofv3 kernel-trace summary.  Every GPU step has its own
# time limit; a crash/abort/timeout stops the script.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${OUT:-run_out}"   # logs and profiles of the session (git-ignored)
mkdir -p "$OUT"
export TMPDIR=/tmp
ok_or_fail() {  # exit codes 0 (pass) and 1 (test failures) continue; anything else stops
  local rc=$1 what=$2
  echo "[$what] rc=$rc"
  if [ "$rc" -ne 0 ] && [ "$rc" -ne 1 ]; then echo "stopping after $what"; exit "$rc"; fi
}
STAGES="${STAGES:-tests bench prof}"
for s in $STAGES; do
  case $s in
    smoke)
      timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke.log 2>&1
      ok_or_fail $? smoke ;;
    tests)
      timeout -k 10 900 python -m pytest tests -m gpu -q -rf ${PYTEST_ARGS:-} > "$OUT"/gpu_tests.log 2>&1
      ok_or_fail $? tests ;;
    bench)
      timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > "$OUT"/bench.json 2> "$OUT"/bench.err
      ok_or_fail $? bench ;;
    prof)
      timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT"/prof -o run --output-format csv -- \
        python3 bench.py --full --steps 5 --warmup 1 --no-cpu --no-c1 > "$OUT"/prof.log 2>&1
      ok_or_fail $? prof ;;
  esac
done
