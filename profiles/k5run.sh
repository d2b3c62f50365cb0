set -o pipefail
O=${1:?usage: profiles/k5run.sh OUTDIR}; mkdir -p "$O"
timeout -k 10 600 python -u -m pytest tests/test_chunk_gpu.py -x -v --timeout 300 --timeout-method thread > $O/pytest.log 2>&1; rc=$?
tail -n 25 $O/pytest.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -u bench.py --full --kernel 5 --steps 3 --warmup 1 --no-cpu > $O/bench5.log 2>&1 || { tail -n 20 $O/bench5.log; exit 1; }
tail -n 1 $O/bench5.log
