#!/usr/bin/env python3
"""Prints VGPR / scratch / occupancy / LDS per kernel of libcocr_hip (hipcc -Rpass-analysis); an argument filters by kernel name
(`ctc_align`, `ctc_spot`, `ctc_spot_graph`, ...: every instantiation of the kernel template is listed)."""
import glob
import os
import re
import subprocess
import sys
import tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
flags = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc', '-mllvm', '-amdgpu-mfma-vgpr-form', '-I', ROOT + '/include',
         '-Rpass-analysis=kernel-resource-usage']
# every translation unit of the library (the host layer's units and the row-chain instantiation units), compiled side by side
with tempfile.TemporaryDirectory() as tmp:
    procs = [subprocess.Popen(flags + ['-c', u, '-o', os.path.join(tmp, os.path.basename(u) + '.o')], stderr=subprocess.PIPE, text=True)
             for u in sorted(glob.glob(ROOT + '/conformer_ocr_amd/csrc/*.hip'))]
    out = ''.join(p.communicate()[1] for p in procs)
cur, rows = None, []
for l in out.splitlines():
    m = re.search(r'Function Name: (\S+)', l)
    if m:
        cur = {'name': m.group(1)}
        rows.append(cur)
        continue
    for key, pat in (('V', 'VGPRs'), ('A', 'AGPRs'), ('scr', r'ScratchSize \[bytes/lane\]'), ('occ', r'Occupancy \[waves/SIMD\]'),
                     ('lds', r'LDS Size \[bytes/block\]')):
        m = re.search(r'remark: .*?\b' + pat + r': (\d+)', l)
        if m and cur is not None:
            cur[key] = m.group(1)
flt = sys.argv[1] if len(sys.argv) > 1 else ''
for r in rows:
    n = subprocess.run(['c++filt', r['name']], capture_output=True, text=True).stdout.strip()
    n = re.sub(r'\(.*', '', n)
    if flt in n:
        print(f"{n[:120]:120s} V{r.get('V')} A{r.get('A')} scr{r.get('scr')} occ{r.get('occ')} lds{r.get('lds')}")
