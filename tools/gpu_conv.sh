#!/bin/bash
# usage: bash tools/gpu_conv.sh OUTDIR
O=${1:?usage: bash tools/gpu_conv.sh OUTDIR}
mkdir -p "$O"
export TMPDIR=/tmp
( timeout 400 python tools/conv_bench.py ) > $O/conv_bench.log 2>&1; echo "conv_bench rc=$?"
( timeout 900 python -m pytest tests -m gpu -q -s ) > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?"
( timeout 300 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline ) > $O/bench_graph.log 2>&1; echo "bench graph rc=$?"
grep -E "passed|failed|FAILED|^E  " $O/pytest_gpu.log | tail -12
grep -E "bench\]" $O/bench_graph.log; tail -c 2500 $O/bench_graph.log | head -c 2400; echo
cat $O/conv_bench.log | python -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d = json.loads(l); print('%-28s err %.1e fwd %6.3f ms %5.1f TF (miopen %5.1f) | f+b %6.3f ms %5.1f TF (miopen %5.1f)' % (d['layer'], d['relerr'], d['hip_fwd_ms'], d['hip_fwd_tf'], d['miopen_fwd_tf'], d['hip_fwdbwd_ms'], d['hip_fwdbwd_tf'], d['miopen_fwdbwd_tf']))
    else: print(l.strip())
"
