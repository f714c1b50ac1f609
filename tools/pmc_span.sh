#!/bin/bash
# SQ issue counters of the span pass (hit_span.hip) on resident input, one rocprofv3 counter run per pass and
# no tracing beside them:
#   bash tools/pmc_span.sh <config> <outdir> [max-errors]
cfg=$1; out=$2; E=${3:-2}
cd "$(dirname "$0")/.." || exit 1
mkdir -p $out; i=0
for c in "SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_SALU SQ_INSTS_SALU SQ_BUSY_CU_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY" \
         "SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_BRANCH SQ_INSTS_LDS SQ_WAIT_INST_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_CYCLES" \
         "SQ_ACTIVE_INST_MISC SQ_INSTS_VALU SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_VALU2 SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_BUSY_CYCLES SQ_WAVES"; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --pmc $c -d $out/pass$i -o run -- python3 tools/kernel_run.py --config $cfg --max-errors $E \
      --positions --spans --launches 2 > $out/pass$i.log 2>&1 || exit 1
done
python3 tools/pmc_kernels.py $out --match hit_start_positions
