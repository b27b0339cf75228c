#!/bin/bash
# Per-dispatch k_huff times of one headline step under a rocprofv3 kernel
# trace (a run of its own: tracing slows the host, so no step time is taken
# from it).  Writes $OUT_DIR/huff_trace_<TAG>.txt (default: build/huff_trace).
#   TAG=new scripts/huff_trace.sh            this tree
#   TAG=parent BENCH=<other tree>/bench.py scripts/huff_trace.sh
set -o pipefail
cd "$(dirname "$0")/.."
R=$(pwd)
TAG=${TAG:-run}
BENCH=${BENCH:-$R/bench.py}
OUT_DIR=${OUT_DIR:-$R/build/huff_trace}
TMP=$(mktemp -d /tmp/huff_trace.XXXXXX)
mkdir -p "$OUT_DIR"
(cd /tmp && timeout -k 10 ${T_PROF:-400} rocprofv3 --kernel-trace --output-format csv -d "$TMP" -o run -- \
    python3 "$BENCH" --gpus 1 --steps 3 --warmup 2 ${BENCH_ARGS} > "$OUT_DIR/huff_trace_${TAG}.out" 2>&1) \
    || { echo "rocprofv3 failed rc=$?"; tail -20 "$OUT_DIR/huff_trace_${TAG}.out"; exit 1; }
CSV=$(find "$TMP" -name '*kernel_trace.csv' | head -1)
[ -n "$CSV" ] || { echo "no kernel trace under $TMP"; exit 1; }
python3 scripts/huff_trace.py "$CSV" ${N_HUFF:-12} | tee "$OUT_DIR/huff_trace_${TAG}.txt"
rm -rf "$TMP"
