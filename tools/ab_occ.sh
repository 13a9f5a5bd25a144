# A/B of herro_find_overlaps' fixed cut between two builds of the library on one GPU box, and the cut taken from the index beside it
# (OLD=/path/to/the/other/libherro_amd.so bash tools/ab_occ.sh; results under ${OUT:-bench_out}/occ).  The two builds run in turn, twice
# each, so that the spread between two runs of one build stands next to the difference between the builds.
out=${OUT:-bench_out}/occ   # OUT: where the results go
mkdir -p $out
run() { name=$1; shift; env "$@" timeout -k 10 300 python tools/overlaprate.py --long-targets 0 --no-align --reps 5 > $out/$name.json 2> $out/$name.err || exit 1; }
if [ -n "$OLD" ]; then
  run fixed_old_1 HERRO_LIB=$OLD
  run fixed_new_1 A=1
  run fixed_old_2 HERRO_LIB=$OLD
  run fixed_new_2 A=1
fi
timeout -k 10 300 python tools/overlaprate.py --long-targets 0 --no-align --reps 5 --occ-frac-ppm ${PPM:-5000} > $out/frac_bench.json 2> $out/frac_bench.err || exit 1
timeout -k 10 300 python tools/overlaprate.py --deep --no-align --reps 5 --occ-frac-ppm ${PPM:-5000} > $out/frac_deep.json 2> $out/frac_deep.err || exit 1
grep -H seconds_median $out/*.json | sed 's/"params".*"seconds_median"/"seconds_median"/' | cut -c1-260
