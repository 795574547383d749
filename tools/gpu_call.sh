#!/bin/bash
# The GPU legs of a check in one command, on the GPU machine.  Logs under $OUT (default out/).
# usage: bash tools/gpu_call.sh TAG [newtests] [tests] [alltests] [bench] [fault] [tptests] [smoke]
TAG=${1:-r3}; shift
WHAT="${*:-alltests bench}"
OUT=${OUT:-out}
mkdir -p $OUT
export TMPDIR=/tmp
PT="python -m pytest -q -p no:cacheprovider"
for w in $WHAT; do
  case $w in
    newtests) timeout 1500 $PT tests/test_hip_long_context_oracle.py tests/test_hip_c5_shape.py "tests/test_hip_tp_p2p.py::test_q4_1_body_with_a_q6_k_classifier_over_the_p2p_group" > $OUT/new_tests_$TAG.log 2>&1; echo "newtests rc=$?"; tail -25 $OUT/new_tests_$TAG.log ;;
    tests) timeout 1500 $PT tests -m gpu --maxfail=25 --deselect tests/test_hip_long_context_oracle.py --deselect tests/test_hip_c5_shape.py > $OUT/gpu_tests_$TAG.log 2>&1; echo "tests rc=$?"; tail -8 $OUT/gpu_tests_$TAG.log ;;
    alltests) timeout 2400 $PT tests -m gpu --maxfail=25 > $OUT/gpu_tests_all_$TAG.log 2>&1; echo "alltests rc=$?"; tail -8 $OUT/gpu_tests_all_$TAG.log ;;
    bench) timeout 900 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err; echo "bench rc=$?"; cat $OUT/bench_$TAG.json; tail -3 $OUT/bench_$TAG.err ;;
    fault) timeout 900 $PT tests/test_hip_fault_paths.py > $OUT/fault_tests_$TAG.log 2>&1; echo "fault rc=$?"; tail -15 $OUT/fault_tests_$TAG.log ;;
    tptests) timeout 900 $PT tests/test_hip_tp.py tests/test_hip_tp_p2p.py > $OUT/tp_tests_$TAG.log 2>&1; echo "tptests rc=$?"; tail -15 $OUT/tp_tests_$TAG.log ;;
    smoke) timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1; echo "smoke rc=$?"; tail -3 $OUT/smoke_$TAG.log ;;
  esac
done
