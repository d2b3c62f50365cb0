set -o pipefail
O=${1:?usage: profiles/k0sort.sh OUTDIR}; mkdir -p "$O"
timeout -k 10 300 python -u -m pytest tests/test_camera_gpu.py -x -q --timeout 200 --timeout-method thread -k "sort or render" > $O/pytest.log 2>&1 || { tail -n 30 $O/pytest.log; exit 1; }
tail -n 2 $O/pytest.log
timeout -k 10 300 python -u bench.py --full --steps 3 --warmup 1 --no-cpu > $O/bench_sort1.log 2>&1 || { tail -n 20 $O/bench_sort1.log; exit 1; }
tail -n 1 $O/bench_sort1.log | cut -c1-700
