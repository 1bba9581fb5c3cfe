#!/bin/bash
# SQ counter passes over bench.py --full (decoder focus). usage (on the MI355X): bash tools/pmc_decoder.sh <tag> [output root, default pmc_out]
set -e
tag=${1:-x}
o=${2:-pmc_out}/pmc_$tag
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $o
rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS -d $o/a -o a --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu --no-latency > $o/a.log 2>&1
rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_INSTS_SALU SQ_INSTS_SMEM SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_INST_CYCLES_SALU -d $o/b -o b --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu --no-latency > $o/b.log 2>&1
python3 profiles/summarize_pmc.py $o/a $o/b > $o/summary.csv
grep ldpc $o/summary.csv
