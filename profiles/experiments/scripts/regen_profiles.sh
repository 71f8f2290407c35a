# usage: bash profiles/experiments/scripts/regen_profiles.sh <output directory>   (from the repository root)
set -e
O=${1:?usage: regen_profiles.sh <output directory>}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $O/gpu_tests.log 2>&1; tail -2 $O/gpu_tests.log
timeout -k 10 600 bash profiles/pmc_pass.sh $O/pmc
python3 profiles/pmc_summarise.py $O/pmc $O/pmc_summary.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -- python3 bench.py --full --no-extra --no-cpu-baseline > $O/bench_under_rocprof.json 2> $O/kt.err
python3 profiles/trace_headline.py $O/kt $O/trace_headline.csv
find $O/kt -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats.csv \;
find $O/kt -name "*kernel_trace.csv" -delete
find $O/pmc -name "*.csv" -size +2M -delete
cat $O/bench_under_rocprof.json | tail -1 | cut -c1-600
