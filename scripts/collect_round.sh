set -x
T=$1
O=${OUT_ROOT:-collect_out}  # output root, shared with scripts/collect_profiles.sh
mkdir -p $O
bash scripts/collect_profiles.sh ${T} 200 full > $O/${T}_collect.log 2>&1
python scripts/lookahead_trace.py 200 > $O/${T}/${T}_lookahead_trace.txt 2>&1
python bench.py --full > $O/${T}/${T}_full_bench.json 2> $O/${T}/full_bench.err
bash scripts/collect_profiles.sh ${T}_N500 500 > $O/${T}_N500_collect.log 2>&1
python scripts/lookahead_trace.py 500 > $O/${T}_N500/${T}_N500_lookahead_trace.txt 2>&1
bash scripts/collect_profiles.sh ${T}_N50 50 > $O/${T}_N50_collect.log 2>&1
python tests/run_configs.py > $O/${T}/${T}_configs.json 2> $O/${T}/configs.err
python scripts/soak_sizes.py > $O/${T}/${T}_size_sweep.txt 2>&1
python bench.py --config batch8 > $O/${T}/${T}_batch8_1rank.json 2>> $O/${T}/full_bench.err
EQVIO_BENCH_ONE_DEVICE=1 python bench.py --config batch8 --gpus 8 > $O/${T}/${T}_batch8_8ranks_one_device.json 2>> $O/${T}/full_bench.err
EQVIO_BENCH_ONE_DEVICE=1 python bench.py --full --gpus 8 --steps 3000 --warmup 300 > $O/${T}/${T}_8ranks_one_device.json 2>> $O/${T}/full_bench.err
tail -c 200 $O/${T}/${T}_full_bench.json
