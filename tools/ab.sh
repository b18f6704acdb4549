# A/B helpers for one GPU session (source this from the repo root; results under $AB_OUT/ab_<name>.*, bench_outputs/ by default):
#     source tools/ab.sh && run base && run three BITHTM_LEAN=1 && runlarge large_c128 BITHTM_LEAN2_CLASSIFY=128
# run: the headline at the default arguments, 3 repetitions, with the per-launch times of --full but none of its legs;
# runlarge: the large_pool leg alone.  Each prints the median rate and the per-launch times of the timed schedule.  Variants are
# environment knobs or another build of the library (BITHTM_LIBRARY=$PWD/bithtm_amd/<other>.so); join the
# calls with && so that nothing follows a run that was killed.
set -e
AB_OUT=${AB_OUT:-bench_outputs}
mkdir -p "$AB_OUT"
run() { # name, env...
  name=$1; shift
  env "$@" timeout -k 10 150 python bench.py --steps 2000 --warmup 500 --reps 3 --full --no-cpu-baseline --no-stress --no-large-pool --no-host-fed > "$AB_OUT/ab_$name.json" 2> "$AB_OUT/ab_$name.err"
  echo "$name: $(grep -o 'median [0-9]* timesteps/s' "$AB_OUT/ab_$name.err" | head -1) | $(grep -o 'launches of the timed schedule.*' "$AB_OUT/ab_$name.err" | head -1 | cut -c1-200)"
}
runlarge() { # name, env...
  name=$1; shift
  env "$@" timeout -k 10 250 python bench.py --large-pool-only --steps 500 --warmup 100 --no-cpu-baseline > "$AB_OUT/ab_$name.json" 2> "$AB_OUT/ab_$name.err"
  echo "$name: $(grep -o 'median [0-9]* timesteps/s' "$AB_OUT/ab_$name.err" | head -1) | $(grep -o 'launches of the timed schedule.*' "$AB_OUT/ab_$name.err" | head -1 | cut -c1-200)"
}
rundriver() { # name, env...: the driver's arguments (20 timed steps per call), 15 repetitions, a plain run
  name=$1; shift
  env "$@" timeout -k 10 150 python bench.py --steps 20 --warmup 5 > "$AB_OUT/ab_$name.json" 2> "$AB_OUT/ab_$name.err"
  echo "$name: $(grep -o 'median [0-9]* timesteps/s (min [0-9]*, max [0-9]*)' "$AB_OUT/ab_$name.err" | head -1)"
}
