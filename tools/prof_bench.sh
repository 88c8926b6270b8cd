# rocprofv3 passes of the default bench command; summaries are copied into profiles/ by hand.
# Everything is written under $PROF_OUT (default prof_out/).
export TMPDIR=/tmp
TAG=${1:-r03}
P=${PROF_OUT:-prof_out}
mkdir -p $P
timeout 1400 rocprofv3 --kernel-trace --stats --output-format csv -d $P/prof_$TAG -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extras > $P/bench_prof_$TAG.log 2>&1
grep "^{\"metric\"" $P/bench_prof_$TAG.log > $P/bench_prof_$TAG.json
timeout 1400 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $P/pmc_fetch_$TAG -- python3 bench.py --steps 1 --warmup 1 > $P/pmc_fetch_$TAG.log 2>&1
timeout 1400 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $P/pmc_write_$TAG -- python3 bench.py --steps 1 --warmup 1 > $P/pmc_write_$TAG.log 2>&1
python3 tools/pmc_traffic.py $P/pmc_fetch_$TAG $P/pmc_write_$TAG > $P/traffic_$TAG.json
cat $P/traffic_$TAG.json | head -30
