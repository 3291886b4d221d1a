# GPU suite + default bench line + the two-partition emulation:  bash tools/run_checks.sh  (one gpurun call)
cd $GRAFT_REPO_ROOT
out=${OUT:-out}
mkdir -p $out
python3 -m pytest tests -m gpu -x -q > $out/gputests.log 2>&1; echo "gpu tests rc=$?" ; tail -3 $out/gputests.log
python3 bench.py --full --steps 20 --warmup 5 > $out/bench_full.json 2> $out/bench_full.err; echo "bench rc=$?"; tail -c 1500 $out/bench_full.err
python3 tools/shard_step_emul.py --mode both > $out/shard_emul.log 2>&1; echo "emul rc=$?"; tail -12 $out/shard_emul.log
