#   bash profiles/h2_check.sh [output directory]
OUT=${1:-profiles/out/h2t}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 400 python -u -m pytest tests/test_gpu_h2.py tests/test_gpu_planes.py -x -q -rfs --timeout 200 --timeout-method thread > "$OUT/pytest.txt" 2>&1
rc=$?; tail -15 "$OUT/pytest.txt"
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python bench.py --full --no-cpu-baseline > "$OUT/bench.log" 2>&1 || { tail -20 "$OUT/bench.log"; exit 1; }
tail -1 "$OUT/bench.log"
