#!/bin/bash
# Run ON THE GPU BOX: FSRCNN x2 720p (4 frames per step) under two builds of the library, one process per run, interleaved.
# usage: bash tools/fs_lib_ab.sh <old.so> [rounds=3]      (the second build is the in-tree product library)
OLD=$1; R=${2:-3}
one() {  # $1 = label, $2 = library path or "", $3 = workload
  SS4K_LIB=$2 python3 bench.py --full --workload $3 --steps 200 --warmup 20 --no-cpu-baseline --no-also 2>/dev/null | python3 -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('%-4s %-11s %7.1f frames/s   stages ms: %s' % ('$1', '$3', d['value'], '  '.join('%s %.4f' % (k.split(' ')[0], v['ms_per_step']) for k, v in d['roofline']['stages'].items())))"
}
for r in $(seq $R); do for wl in fsrcnn_f16 fsrcnn; do one old $OLD $wl; one new "" $wl; done; done
