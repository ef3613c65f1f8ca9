#!/bin/bash
# Runs on an MI355X: kernel-trace stats + separate PMC passes of the bench command (counters in runs of their own, never with API tracing).
#   scripts/profile_gpu.sh TAG [extra bench.py arguments, e.g. --robot human --bs 1024]
# Outputs under gpurun_out/prof_$TAG/ ; scripts/summarize_profile.py turns them into profiles/*.
# PPR_DIFFPHYS_LIB (+ PPR_DIFFPHYS_ANY_ABI=1) profiles another build of the library, e.g. the parent commit's for a before / after pair.
# Every pass runs under its own time limit, and the first one that fails ends the script: nothing more is started on the GPU behind it.
TAG=${1:-r02}
shift
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$REPO/gpurun_out/prof_$TAG
LIMIT=${PROFILE_STEP_SECONDS:-240}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
BENCH="python3 $REPO/bench.py --steps 10 --warmup 2 --repeats 2 --full --no-cpu-baseline --no-boundary $@"
echo "$BENCH" > $OUT/command.txt
# which library these counters are of: the source half of pd_build_id() -- bench.py drops counter-derived fields when it differs from the library it runs
python3 -c "import sys; sys.path.insert(0, '$REPO/ppr-diffphys_amd'); from diffphys_amd import hip_backend; print(hip_backend.build_id().split('+')[-1])" > $OUT/source_hash.txt 2>/dev/null
pass() {  # pass <directory> <log> <rocprofv3 options...>
  local dir=$1 log=$2; shift 2
  timeout -k 10 $LIMIT rocprofv3 --kernel-trace "$@" --output-format csv -d $OUT/$dir -- $BENCH > $OUT/$log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "profile_gpu.sh: pass $dir ended with status $rc"; tail -20 $OUT/$log; exit 1; fi
}
pass trace trace.log --stats
pass pmc_fetch pmc_fetch.log --pmc FETCH_SIZE
pass pmc_write pmc_write.log --pmc WRITE_SIZE
pass pmc_sq pmc_sq.log --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_ACTIVE_INST_ANY
pass pmc_sq2 pmc_sq2.log --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_INST_CYCLES_VMEM GRBM_GUI_ACTIVE
find $OUT -name "*.csv" | head -50 > $OUT/files.txt
# keep the merge small: drop anything that is not a csv/log/txt
find $OUT -type f ! -name "*.csv" ! -name "*.log" ! -name "*.txt" -delete
du -sh $OUT
