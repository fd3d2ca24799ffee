#!/bin/bash
# On the GPU box: profile THE DRIVER'S bench command and assemble profiles/<round> material in $OUT_DIR/.
# usage: tools/gpu_profile_driver_cmd.sh <tag>
set -u
tag=${1:-r03a}
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
: "${OUT_DIR:?set OUT_DIR to the folder the outputs go to}"
mkdir -p "$OUT_DIR"
ARGS="--steps 20 --warmup 5 --no-cpu-baseline --fused-steps 0 --no-measure-traffic --full"
python3 bench.py --steps 20 --warmup 5 --full > $OUT_DIR/${tag}_bench.json 2> $OUT_DIR/${tag}_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/${tag}_trace -o t -- python3 bench.py $ARGS > $OUT_DIR/${tag}_bench_under_trace.json 2> $OUT_DIR/${tag}_trace.err
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT_DIR/${tag}_w -o w -- python3 bench.py $ARGS > $OUT_DIR/${tag}_w.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT_DIR/${tag}_f -o f -- python3 bench.py $ARGS > $OUT_DIR/${tag}_f.log 2>&1
python3 tools/make_profile_summary.py ${tag} auto $OUT_DIR/${tag}_bench_driver_summary.json 20 3 2000 > $OUT_DIR/${tag}_summary.log 2>&1
find $OUT_DIR/${tag}_trace -name '*kernel_stats.csv' -exec cp {} $OUT_DIR/${tag}_kernel_stats.csv \;
# keep the merge-back small: the raw traces are tens of MB
rm -rf $OUT_DIR/${tag}_trace $OUT_DIR/${tag}_w $OUT_DIR/${tag}_f
python3 bench.py --full > $OUT_DIR/${tag}_bench_default.json 2>> $OUT_DIR/${tag}_bench.err
tail -c 1500 $OUT_DIR/${tag}_bench.json
tail -c 1600 $OUT_DIR/${tag}_summary.log
