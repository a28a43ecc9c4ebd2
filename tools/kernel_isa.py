#!/usr/bin/env python3
"""Prints a sha256 of the compiled gfx950 code of every kernel of the library, by kernel name (the default) or of the given .hip
units, unit by unit.

    tools/kernel_isa.py [--against OTHER_CSRC_DIR] [--json OUT] [--by-name | unit.hip ...]

Each unit is compiled with the flags of build.py (COCR_HIPCC_FLAGS included) plus --offload-device-only -S.  The assembly is
normalised -- comment lines, trailing `;` comments, .file and .ident dropped, __hip_cuid_<hex> made a constant, the number of
the function inside its unit taken out of its local labels (.LBB<function>_<block> -> .LBB_<block>, .Lfunc_end<function>: the
number only counts the kernels emitted before this one, the block number that tells the labels of one kernel apart stays, and a
piece holds one kernel, so no two labels fall together) -- and cut into one piece per kernel (code and kernel descriptor).
--against: the units of the same names in another csrc directory (a checkout of another commit) are compiled too and the
kernels that differ, or exist on one side only, are listed; the exit status is 1 if there are any.  A refactor that moves
code verbatim leaves every hash as it is; one that merely looks equivalent usually does not.
--by-name (the default when no unit is named): every *.hip of each tree is compiled and {kernel name: hash} is compared over the
union of a tree's units, for changes that move kernels between units.  A kernel compiled into several units of one tree (a
template two units instantiate alike) must have one hash there; those kernels are listed."""
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


def by_name(dirs, json_out):
    """Every unit of each tree; kernels compared by name over the union of a tree's units."""
    units = {d: sorted(f for f in os.listdir(d) if f.endswith('.hip')) for d in dirs}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as pool:
        jobs = {(d, u): pool.submit(assembly, d, u, tmp) for d in dirs for u in units[d]}
        trees = []
        for d in dirs:                    # {kernel: {hash: [units]}}
            tree = {}
            for u in units[d]:
                for n, h in kernels(jobs[(d, u)].result()).items():
                    tree.setdefault(n, {}).setdefault(h, []).append(u)
            trees.append(tree)
    new, old = trees[0], trees[1] if len(trees) > 1 else None
    names = demangle(sorted(set(new) | set(old or {})))
    one = lambda t, n: sorted(t[n])[0] if n in t else None
    rows, bad = [], 0
    for n in sorted(names, key=names.get):
        row = {'name': names[n], 'sha256': one(new, n), 'units': sorted(u for us in new.get(n, {}).values() for u in us)}
        split = len(new.get(n, {})) > 1 or (old is not None and len(old.get(n, {})) > 1)      # units of one tree disagree
        if old is not None:
            row['against'] = one(old, n)
            row['against_units'] = sorted(u for us in old.get(n, {}).values() for u in us)
        same = not split and (old is None or row['against'] == row['sha256'])
        bad += not same
        rows.append(row)
        print('%s %s %s  [%s]' % ((row['sha256'] or '-' * 64)[:16], '  ' if same else '!=', names[n], ' '.join(u[:-4] for u in row['units'])))
        if not same:
            print('%s    (%s%s)' % ((row.get('against') or '-' * 64)[:16], 'against' if old is not None else '', ', units of one tree disagree' if split else ''))
    dups = [r for r in rows if len(r['units']) > 1]
    print('kernels compiled into several units (%d):' % len(dups))
    for r in dups:
        print('    %s  [%s]' % (r['name'], ' '.join(u[:-4] for u in r['units'])))
    print('%d kernels in %d units' % (len(new), len(units[dirs[0]])) + ('' if old is None else ', %d in the %d units of the other tree, %d differ, are missing or are new'
          % (len(old), len(units[dirs[1]]), bad)))
    if json_out:
        with open(json_out, 'w') as fp:
            json.dump({'kernels': rows, 'several_units': [r['name'] for r in dups]}, fp, indent=1)
            fp.write('\n')
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--against', help='csrc directory of another checkout to compare with')
    ap.add_argument('--json', help='write {unit: [{name, sha256[, against]}]} there')
    ap.add_argument('--by-name', action='store_true', help='every unit of each tree, kernels compared by name (the default when no unit is named)')
    ap.add_argument('units', nargs='*')
    a = ap.parse_args()
    dirs = [CSRC] + ([os.path.abspath(a.against)] if a.against else [])
    if a.by_name or not a.units:
        return by_name(dirs, a.json)
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
