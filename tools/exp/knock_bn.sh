#!/bin/bash
# per-phase knock-outs of the register-resident BatchNorm kernels (`make -C waveformml_amd/csrc knock_bn` builds bn.hip
# with -DWFS_BN_KNOCK=bits: 1 no fold of the partials, 2 no row loads (every thread reads row 0), 4 no row stores,
# 8 no LDS reduction / partial store in the reduce kernel, 16 no shift / running-statistics loads in the forward
# elementwise kernel), timed by tools/microbench_conv.py inside a replayed graph.  Stops at the first run that fails.
cd "$(dirname "$0")/../.."
for kn in base 1 2 4 8 16 3 7 15 23 31 base; do
  if [ $kn = base ]; then unset WFS_LIB; else export WFS_LIB=$PWD/tools/exp/bnk$kn/libwfsparse.so; fi
  out=$(timeout -k 10 300 python tools/microbench_conv.py 50 bf16 2>/dev/null) || { echo "knock $kn: run failed ($?)"; exit 1; }
  echo "knock $kn: $(echo "$out" | grep -E '^bn\+relu' | tr '\n' ' ')"
done
