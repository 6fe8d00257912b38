#!/bin/bash
# Instruction mix of the MX GEMMs (k_gemm_mx_pipe / k_gemm_ring_mx) over one segmentation forward: two counter passes, each a
# run of its own with NO tracing beside it, then instructions executed per MFMA by kind.
# usage: bash tools/pmc_mx_pipe.sh [out dir] [library]   ->   <out dir>/summary.txt
export TMPDIR=/tmp
OUT=${1:-/tmp/pmc_mx_pipe}
[ -n "$2" ] && export AVL_HIP_LIB=$2
case "$OUT" in ""|/|.|..) echo "refusing to use '$OUT' as the output directory"; exit 2;; esac
rm -rf -- "$OUT"; mkdir -p "$OUT"
ARGS="tools/profile_seg.py --reps 1 --top 1 --precision mixed"
timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_SALU SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_SMEM SQ_INSTS_LDS SQ_INSTS_VMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d $OUT/p1 -- python3 $ARGS > $OUT/p1.log 2>&1 || { echo "pass 1 failed"; tail -5 $OUT/p1.log; exit 1; }
timeout -k 10 240 rocprofv3 --pmc SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_MISC SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d $OUT/p2 -- python3 $ARGS > $OUT/p2.log 2>&1 || { echo "pass 2 failed"; tail -5 $OUT/p2.log; exit 1; }
python3 tools/pmc_mx_pipe_summary.py $OUT | tee $OUT/summary.txt
