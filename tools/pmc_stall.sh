cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
OUT=gpurun_out/r2stall; mkdir -p $OUT
timeout -s KILL 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES --kernel-trace -d $OUT/pmc_stall -o pmc --output-format csv -- python3 bench.py --steps 2 --warmup 1 > $OUT/bench_stall.json 2> $OUT/stall.err || { tail -5 $OUT/stall.err; exit 3; }
timeout -s KILL 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM SQ_WAIT_INST_LDS SQ_INST_CYCLES_VMEM SQ_WAVES --kernel-trace -d $OUT/pmc_mix -o pmc --output-format csv -- python3 bench.py --steps 2 --warmup 1 > $OUT/bench_mix.json 2> $OUT/mix.err || { tail -5 $OUT/mix.err; exit 3; }
echo done
