#!/bin/bash
# kernel resource usage of one .hip file (registers, scratch, LDS, occupancy): bash tools/kres.sh csrc/file.hip [extra flags]
f=$1; shift
obj=$(mktemp --suffix=.o) || exit 1
trap 'rm -f "$obj"' EXIT
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c "$f" -o "$obj" -Rpass-analysis=kernel-resource-usage "$@" 2>&1 | python3 -c "
import sys,re
KEYS={'SGPRs:':'SGPRs','VGPRs:':'VGPRs','AGPRs:':'AGPRs','ScratchSize':'Scratch','Occupancy':'Occupancy','LDS Size':'LDS',
      'SGPRs Spill':'SGPRspill','VGPRs Spill':'VGPRspill'}
for l in sys.stdin:
    m=re.search(r'Function Name: (\S+)',l)
    if m: print(); print(m.group(1)[:90],end=' ')
    if 'error:' in l: print(); print(l.rstrip())
    for k,label in KEYS.items():
        m=re.search(re.escape(k)+r'\D*(\d+)',l)          # the whole number: the digits start where the non-digits end
        if m: print(label+'='+m.group(1),end=' ')
print()
"
