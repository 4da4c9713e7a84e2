#!/bin/bash
# Where a wave of k_tall_spmv waits: SQ counters of the two products of config 4 alone
# (tools/c4_products_only.py: every k_tall_spmv launch is a whole product), each counter set in a run of its own with no tracing
# beside it, plus FETCH_SIZE per launch.  -> OUTDIR/prof_tall_pipeline_NAME/{sq1,sq2,sq3}.json, fetch.json
#     tools/profile_tall_pipeline.sh NAME [OUTDIR]   (OUTDIR: default prof_out; SLP_LIB_VARIANT in the environment chooses the library)
# Every step runs under a time limit of its own and the first one that fails ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
O=${2:-prof_out}/prof_tall_pipeline_${1:?name}
mkdir -p $O
export TMPDIR=/tmp
SQ1="SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT"
SQ2="SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_BUSY_CYCLES"
SQ3="SQ_WAVE_CYCLES SQ_WAIT_INST_LDS SQ_INST_CYCLES_SALU SQ_INST_CYCLES_SMEM SQ_INST_CYCLES_VMEM_RD SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_MISC SQ_LDS_ADDR_CONFLICT"
run() {   # run NAME COUNTERS...
    local n=$1; shift
    timeout -k 10 240 rocprofv3 --pmc "$@" -d "$(realpath $O)/$n" -o $n -- python3 tools/c4_products_only.py 2 > $O/$n.out 2> $O/$n.err || { echo "$n: exit $?"; tail -5 $O/$n.err; return 1; }
}
run sq1 $SQ1 && run sq2 $SQ2 && run sq3 $SQ3 && run fetch FETCH_SIZE || exit 1
for n in sq1 sq2 sq3 fetch; do
    python3 tools/summarize_rocprof.py db-sq $(find $O/$n -name "*.db" | head -1) > $O/$n.json
    rm -rf $O/$n
done
grep -A14 "k_tall_spmv" $O/sq1.json $O/sq2.json $O/sq3.json $O/fetch.json | grep -v "^--"
