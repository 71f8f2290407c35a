# usage: bash profiles/experiments/scripts/regen_full_bench_profiles.sh <output directory>   (from the repository root)
set -e
O=${1:?usage: regen_full_bench_profiles.sh <output directory>}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/ktfull -- python3 bench.py --full > $O/bench_full_under_rocprof.json 2> $O/ktfull.err
find $O/ktfull -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_full.csv \;
rm -rf $O/ktfull
timeout -k 10 600 python3 bench.py --full > $O/bench.json 2> $O/bench.err
timeout -k 10 600 python3 bench.py --gpus 1 --spawn --full > $O/bench_spawn.json 2> $O/bench_spawn.err || true
tail -c 300 $O/bench.json
