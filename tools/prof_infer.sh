# rocprofv3 kernel stats of the inference post-process bench; summary copied into profiles/ by hand.
# Everything is written under $PROF_OUT (default prof_out/).
export TMPDIR=/tmp
TAG=${1:-r03}
P=${PROF_OUT:-prof_out}
mkdir -p $P
python3 tools/bench_infer.py --frames 2048 > $P/infer_$TAG.json 2> $P/infer_$TAG.err
tail -3 $P/infer_$TAG.err
cat $P/infer_$TAG.json
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $P/prof_infer_$TAG -- python3 tools/bench_infer.py --frames 1024 --cpu-frames 0 > $P/infer_prof_$TAG.log 2>&1
tail -2 $P/infer_prof_$TAG.log
f=$(ls $P/prof_infer_$TAG/*/*kernel_stats.csv | head -1)
head -25 $f | cut -c1-200
