#!/bin/bash
# development helper (GPU box): rocprofv3 kernel statistics of the forward-only bench -> prof_out/r04_fwd_kernel_stats.csv (or $PROF_OUT)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${PROF_OUT:-$R/prof_out}; mkdir -p $O
rm -rf /tmp/prof_fwd
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_fwd -- python3 $R/bench.py --full --forward-only --steps 20 --warmup 3 --no-cpu-baseline --no-extra > $O/r04_fwd_prof_bench.json 2> $O/r04_fwd_prof_bench.err
f=$(find /tmp/prof_fwd -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $O/r04_fwd_kernel_stats.csv
head -30 $O/r04_fwd_kernel_stats.csv | cut -c1-200
