# A/B of the end_to_end leg on the GPU box: feeder modes x host pool sizes, with the cgroup throttling counters around each run
# (bash tools/ab_e2e.sh; results under ${OUT:-bench_out}/r2o).
out=${OUT:-bench_out}/r2o   # OUT: where the results go
mkdir -p $out
thr() { grep -E "nr_throttled|throttled_usec|usage_usec" /sys/fs/cgroup/cpu.stat | tr '\n' ' '; echo; }
HOSTPREP_THREADS=1,4,8,16,32,64 python tools/hostprep_cpu.py 1024 > $out/hostprep.log 2>&1
run() { name=$1; shift; echo "== $name before: $(thr)" >> $out/thr.log; env "$@" python bench.py --full --no-cpu-baseline --self-check 0 --e2e-jobs 8 --e2e-mode $MODE > $out/$name.json 2> $out/$name.err; echo "== $name after: $(thr)" >> $out/thr.log; }
MODE=serial run serial_def A=1
MODE=producer run producer_def A=1
MODE=serial run serial_t8 HERRO_HOST_THREADS=8
MODE=producer run producer_t8 HERRO_HOST_THREADS=8
MODE=serial run serial_t64 HERRO_HOST_THREADS=64
cat $out/thr.log; tail -8 $out/hostprep.log
