#!/bin/bash
# Round-2 profile (run ON the GPU box): bench line; rocprofv3 kernel-trace stats of the bench, of the 500-family batches
# (W = 40 and 80) and of BASELINE config 2 (N = 1,000 x L = 2,000, device-wide cell-parallel kernel); PMC passes (one
# counter set per run, no tracing) for the persistent kernel of the bench and for the cell-parallel kernels.
TAG=${1:-r02}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=gpurun_out/$TAG; rm -rf $O; mkdir -p $O
python3 bench.py --full > $O/bench.json 2> $O/bench.err; tail -c 600 $O/bench.json; echo
stats() {  # name, command...
  local name=$1; shift
  rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$name -- "$@" > $O/trace_$name.out 2> $O/trace_$name.err
  echo "$name: exit $? ($(grep -c SIGSEGV $O/trace_$name.err) SIGSEGV)"
  f=$(find $O/trace_$name -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $O/kernel_stats_$name.csv && head -6 $O/kernel_stats_$name.csv
  rm -rf $O/trace_$name
}
stats bench python3 bench.py --full --steps 1 --warmup 1 --no-cpu --no-seam1
stats batch_w40 python3 tools/bench_batch.py 500 40
stats batch_w80 python3 tools/bench_batch.py 500 80
stats cfg2 python3 tools/cp_dev_timing.py 1000
pmc() {  # name, command...
  local name=$1; shift
  local i=0
  for set in \
    "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_BUSY_CYCLES" \
    "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT" \
    "FETCH_SIZE" "WRITE_SIZE" "GRBM_GUI_ACTIVE" ; do
    i=$((i+1))
    rocprofv3 --pmc $set --output-format csv -d $O/pmc_$name/pass$i -- "$@" > $O/pmc_$name.pass$i.log 2>&1 || echo "pmc $name pass $i: non-zero exit"
  done
  python3 tools/pmc_summary2.py $O/pmc_$name > $O/pmc_$name.json; rm -rf $O/pmc_$name $O/pmc_$name.pass*.log
  echo "pmc $name done"
}
pmc bench python3 bench.py --steps 1 --warmup 0 --no-cpu --no-seam1 --L 256
pmc batch_w40 python3 tools/bench_batch.py 500 40
pmc cfg2 python3 tools/cp_dev_timing.py 1000
ls $O
