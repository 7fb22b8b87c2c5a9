#!/bin/bash
# Dev: registers / spills / scratch / static LDS of every kernel whose name holds the filter (default: onf_x32_kernel) in a
# built library (default: the product library).  Usage: tools/x32/kernel_regs.sh [lib] [name filter]
L=${1:-$(cd "$(dirname "$0")/../.." && pwd)/pytorch-motion-planner_amd/nfopp/lib/libnfopp_hip.so}
T=$(mktemp -d); cp "$L" $T/lib.so; cd $T
/opt/rocm/lib/llvm/bin/llvm-objdump --offloading lib.so >/dev/null 2>&1
for f in *gfx950*; do /opt/rocm/lib/llvm/bin/llvm-readelf --notes "$f" | python3 -c "
import sys,re
t=sys.stdin.read()
for block in re.split(r'\n  - (?=\.)', t):      # one entry of amdhsa.kernels each
    f=dict(re.findall(r'^\s*\.(\w+):\s+(\S+)', block, re.M))
    if 'vgpr_count' in f and '${2:-onf_x32_kernel}' in f.get('name',''):
        print(f['name'][:72], 'scratch',f['private_segment_fixed_size'],'sgpr',f['sgpr_count'],'vgpr',f['vgpr_count'],
              'spill',int(f['vgpr_spill_count'])+int(f['sgpr_spill_count']),'lds',f['group_segment_fixed_size'])
"; done
rm -rf $T
