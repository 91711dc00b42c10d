#!/bin/bash
# full GPU suite + smoke + the full bench (the driver's round-end sequence); tag = $1, output directory = $2
set -o pipefail
tag=${1:-r5}
out=${2:-bench_out}
mkdir -p $out
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread \
  > $out/${tag}_gpu_tests.log 2>&1 || exit $?
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $out/${tag}_smoke.log 2>&1 || exit $?
timeout -k 10 600 python bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err
