#!/bin/bash
# Static figures of the tall-cell product kernel for the candidates of DESIGN section 3 (x): item depth DI, tile depth DT, the
# next packet's value reads in front of its barrier (AHEAD).  Compiles pysparselp_amd/csrc/slp_tall_spmv.hip to assembly with
# the Makefile's flags and the lab overrides (-DSLP_LAB_VARIANT -DSLP_TALL_DI= -DSLP_TALL_DT= -DSLP_TALL_AHEAD=), then prints
# NumVgprs / scratch / occupancy and tools/lab/count_loop.py's table for the two bodies the benchmark's LP runs on.
#     tools/lab/tall_pipeline_variants.sh OUTDIR ["DI,DT,AHEAD" ...]
set -o pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
SRC="$HERE/../../pysparselp_amd/csrc"
OUT="${1:?output directory}"; shift
mkdir -p "$OUT"
CANDS=("$@")
[ ${#CANDS[@]} -eq 0 ] && CANDS=("4,4,0" "4,2,0" "4,3,0" "6,2,0" "6,3,0" "8,2,0" "4,4,1" "4,2,1" "4,3,1")
for c in "${CANDS[@]}"; do
    IFS=, read -r di dt ah <<< "$c"
    s="$OUT/tall_di${di}_dt${dt}_a${ah}.s"
    ${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I/opt/rocm/include -mllvm -amdgpu-sched-strategy=max-ilp \
        -DSLP_LAB_VARIANT -DSLP_TALL_DI=$di -DSLP_TALL_DT=$dt -DSLP_TALL_AHEAD=$ah --cuda-device-only -S "$SRC/slp_tall_spmv.hip" -o "$s" 2> /dev/null || { echo "DI=$di DT=$dt AHEAD=$ah: does not compile"; continue; }
    for body in k_tall_spmvILb1ELb0ELb0ELi3072ELb1E k_tall_spmvILb1ELb0ELb0ELi4096ELb1E; do
        echo "DI=$di DT=$dt AHEAD=$ah $body"
        python3 "$HERE/count_loop.py" "$s" $body | grep -E "loop with|NumVgprs|ScratchSize|Occupancy"
    done
done
