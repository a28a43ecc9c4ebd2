#!/usr/bin/env python3
"""Prints a sha256 of the compiled gfx950 code of every kernel of the given .hip units (default: the three row-chain units).

    tools/kernel_isa.py [--against OTHER_CSRC_DIR] [--json OUT] [unit.hip ...]

Each unit is compiled with the flags of build.py (COCR_HIPCC_FLAGS included) plus --offload-device-only -S.  The assembly is
normalised -- comment lines, trailing `;` comments, .file and .ident dropped, __hip_cuid_<hex> made a constant, the number of
the function inside its unit taken out of its local labels (.LBB<function>_<block> -> .LBB_<block>, .Lfunc_end<function>: the
number only counts the kernels emitted before this one, the block number that tells the labels of one kernel apart stays, and a
piece holds one kernel, so no two labels fall together) -- and cut into one piece per kernel (code and kernel descriptor).
--against: the units of the same names in another csrc directory (a checkout of another commit) are compiled too and the
kernels that differ, or exist on one side only, are listed; the exit status is 1 if there are any.  A refactor that moves
code verbatim leaves every hash as it is; one that merely looks equivalent usually does not."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'conformer_ocr_amd', 'csrc')
UNITS = ['rowchain_d256.hip', 'rowchain_d256_head.hip', 'rowchain_d512.hip']


def assembly(csrc, unit, tmp):
    include = os.path.join(csrc, '..', '..', 'include')
    out = os.path.join(tmp, '%s.%s.s' % (hashlib.sha256(csrc.encode()).hexdigest()[:8], unit))
    cmd = ['/opt/rocm/bin/hipcc'] + os.environ.get('COCR_HIPCC_FLAGS', '').split() + [
        '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc', '-mllvm', '-amdgpu-mfma-vgpr-form',
        '-DCOCR_SRC_HASH="isa"', '-I', include if os.path.isdir(include) else os.path.join(ROOT, 'include'),
        '--offload-device-only', '-S', os.path.join(csrc, unit), '-o', out]
    subprocess.check_call(cmd)
    with open(out) as fp:
        return fp.read()


def kernels(text):
    """{mangled kernel name: sha256 of its normalised assembly}"""
    lines = []
    for l in text.split('.amdgpu_metadata')[0].splitlines():
        l = l.split(';')[0].rstrip()
        if not l.strip() or re.match(r'\s*\.(file|ident)\b', l):
            continue
        l = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_0', l)
        lines.append(re.sub(r'\.L(BB|func_begin|func_end)\d+', r'.L\1', l))
    out, name, body = {}, None, []
    for l in lines:                       # a kernel: from its .type line to the end of its descriptor (what follows names its neighbour)
        m = re.match(r'\s*\.type\s+(\S*),@function', l)
        if m:
            name, body = m.group(1), []
        body.append(l)
        if name and '.end_amdhsa_kernel' in l:
            out[name] = hashlib.sha256('\n'.join(body).encode()).hexdigest()
            name = None
    return out


def demangle(names):
    res = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r'^void ', '', re.sub(r'\(.*', '', d)) for n, d in zip(names, res)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--against', help='csrc directory of another checkout to compare with')
    ap.add_argument('--json', help='write {unit: [{name, sha256[, against]}]} there')
    ap.add_argument('units', nargs='*', default=UNITS)
    a = ap.parse_args()
    dirs = [CSRC] + ([os.path.abspath(a.against)] if a.against else [])
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=6) as pool:
        jobs = {(d, u): pool.submit(assembly, d, os.path.basename(u), tmp) for d in dirs for u in a.units}
        hashes = {k: kernels(j.result()) for k, j in jobs.items()}
    differ, report = 0, {}
    for u in a.units:
        new, old = hashes[(CSRC, u)], hashes.get((dirs[-1], u)) if a.against else None
        names = demangle(sorted(set(new) | set(old or {})))
        report[u] = rows = []
        for n in sorted(names, key=names.get):
            row = {'name': names[n], 'sha256': new.get(n)}
            if old is not None:
                row['against'] = old.get(n)
            rows.append(row)
            same = old is None or old.get(n) == new.get(n)
            differ += not same
            print('%s %s %s' % ((new.get(n) or '-' * 64)[:16], '  ' if same else '!=', names[n]))
            if not same:
                print('%s    (%s)' % ((old.get(n) or '-' * 64)[:16], 'against'))
        print('%s: %d kernels' % (u, len(new)) + ('' if old is None else ', %d of the other tree, %d differ or are missing'
              % (len(old), sum(r['sha256'] != r['against'] for r in rows))))
    if a.json:
        with open(a.json, 'w') as fp:
            json.dump(report, fp, indent=1)
            fp.write('\n')
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
