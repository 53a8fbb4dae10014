# bench.py --gpus 2 --full rehearsed on ONE GPU: both ranks on device 0, exchange through the host-staged transport (gloo)
OUT=${1:-bench_out/rehearse_two_ranks}
mkdir -p $OUT
LSA_BENCH_STACKS=${LSA_BENCH_STACKS:-90} LSA_BENCH_DEVICE=0 LSA_BENCH_BACKEND=gloo timeout -k 10 ${REHEARSE_TIMEOUT:-300} python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus 2 --steps 2 --warmup 1 --full > $OUT/bench_2ranks_rehearsal.json 2> $OUT/bench_2ranks.err
echo "exit $?"
grep -v "^\[W\|amdgpu.ids" $OUT/bench_2ranks.err | tail -60
python3 tools/print_bench_line.py $OUT/bench_2ranks_rehearsal.json
