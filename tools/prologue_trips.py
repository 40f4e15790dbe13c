#!/usr/bin/env python3
"""Prologue report of the rasterizer's step kernels (CPU only: needs hipcc, no GPU).

Compiles the five kernel files of the step with the flags of ``exavatar_release_amd/build.py`` to gfx950 assembly and
prints, for every kernel instantiation,

  * scalar loads          ``s_load_*`` / ``s_buffer_load_*`` issued before the first vector memory load,
  * serial scalar waits   the ``s_waitcnt`` with an ``lgkmcnt`` field that find at least one of those loads outstanding:
                          scalar loads return out of order, so such a wait is always for ALL of them -- one full round
                          trip each, one after the other,
  * VGPRs, waves per SIMD, scratch bytes per lane and static LDS, as the compiler states them in the listing.

It is a LINEAR scan of the listing (branches are not followed, a load behind a not-taken branch counts), so the numbers
are approximate, and they depend on the compiler: a report to read next to the ISA, not a test.

    python tools/prologue_trips.py                 # the working tree
    python tools/prologue_trips.py --rev HEAD~1    # the sources of a git revision
    python tools/prologue_trips.py --keep DIR      # also leave the listings in DIR
"""
import argparse
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import importlib.util      # build.py by path: its flags only, without importing the package (no torch, nothing built)
_spec = importlib.util.spec_from_file_location('_exa_build', os.path.join(ROOT, 'exavatar_release_amd', 'build.py'))
_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_build)

FILES = ['preprocess_fwd.hip', 'binning.hip', 'render_fwd.hip', 'render_bwd.hip', 'preprocess_bwd.hip']
VMEM_LOAD = re.compile(r'^(global_load|buffer_load|flat_load|scratch_load|global_atomic|buffer_atomic|flat_atomic)')
SMEM_LOAD = re.compile(r'^(s_load_|s_buffer_load_)')


def sources(rev, tmp):
    """csrc/ and include/ of `rev` (None: the working tree) laid out under tmp as in the repository."""
    if rev is None:
        return os.path.join(ROOT, 'exavatar_release_amd', 'csrc')
    for d in ('exavatar_release_amd/csrc', 'include'):
        os.makedirs(os.path.join(tmp, d))
        names = subprocess.run(['git', '-C', ROOT, 'ls-tree', '--name-only', rev, d + '/'], check=True,
                               capture_output=True, text=True).stdout.split()
        for n in names:
            with open(os.path.join(tmp, n), 'wb') as f:
                f.write(subprocess.run(['git', '-C', ROOT, 'show', rev + ':' + n], check=True, capture_output=True).stdout)
    return os.path.join(tmp, 'exavatar_release_amd', 'csrc')


def compile_listing(csrc, name, out):
    cmd = [_build.hipcc()] + _build.COMMON + _build.SOURCES[name] + \
        ['-w', '--cuda-device-only', '-S', os.path.join(csrc, name), '-o', out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def demangle(names):
    filt = shutil.which('llvm-cxxfilt') or os.path.join(os.path.dirname(os.path.realpath(_build.hipcc())), '..', 'llvm', 'bin',
                                                        'llvm-cxxfilt')
    if not os.path.exists(filt):
        filt = shutil.which('c++filt')
    if not filt:
        return dict(zip(names, names))
    out = subprocess.run([filt] + names, check=True, capture_output=True, text=True).stdout.splitlines()
    short = []
    for s in out:
        s = re.sub(r'^void ', '', s)
        s = re.sub(r'\(.*$', '', s)                      # drop the argument list
        short.append(s.replace('exa::', ''))
    return dict(zip(names, short))


def scan(listing):
    """-> [(mangled name, scalar loads, serial waits, resources dict)] in listing order."""
    rows, body, name = [], None, None
    res = {}
    with open(listing) as f:
        lines = f.read().splitlines()
    kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', '\n'.join(lines), re.M))
    i = 0
    while i < len(lines):
        m = re.match(r'^(\w+):', lines[i])
        if m and m.group(1) in kernels:
            name, body, res = m.group(1), [], {}
            i += 1
            while i < len(lines) and not lines[i].strip().startswith('.end_amdhsa_kernel'):
                body.append(lines[i])
                i += 1
            while i < len(lines) and not re.match(r'^; Occupancy', lines[i]):
                for key in ('NumVgprs', 'NumAgprs', 'ScratchSize', 'LDSByteSize'):
                    mm = re.match(r'^; %s: (\d+)' % key, lines[i])
                    if mm:
                        res[key] = int(mm.group(1))
                i += 1
            if i < len(lines):
                res['Occupancy'] = int(re.match(r'^; Occupancy: (\d+)', lines[i]).group(1))
            loads = waits = outstanding = 0
            for ln in body:
                ins = ln.split(';')[0].strip()
                if not ins or ins.endswith(':') or ins.startswith('.'):
                    continue
                if VMEM_LOAD.match(ins):
                    break
                if SMEM_LOAD.match(ins):
                    loads += 1
                    outstanding += 1
                elif ins.startswith('s_waitcnt') and ('lgkmcnt' in ins or re.match(r'^s_waitcnt\s+(0x[0-9a-f]+|\d+)\s*$', ins)):
                    if outstanding:
                        waits += 1
                    outstanding = 0
            rows.append((name, loads, waits, res))
        i += 1
    return rows


def report(rev, keep):
    tmp = tempfile.mkdtemp(prefix='prologue_trips_')
    try:
        csrc = sources(rev, tmp)
        out_dir = keep or os.path.join(tmp, 'asm')
        os.makedirs(out_dir, exist_ok=True)
        print('| file | kernel | scalar loads | serial scalar waits | VGPRs | waves / SIMD | scratch B | static LDS B |')
        print('|---|---|---|---|---|---|---|---|')
        tl = tw = 0
        for name in FILES:
            listing = os.path.join(out_dir, name.replace('.hip', '.s'))
            compile_listing(csrc, name, listing)
            rows = scan(listing)
            names = demangle([r[0] for r in rows])
            for mangled, loads, waits, res in rows:
                tl += loads
                tw += waits
                print('| %s | `%s` | %d | %d | %d | %d | %d | %d |' % (
                    name, names[mangled], loads, waits, res.get('NumVgprs', -1) + res.get('NumAgprs', 0),
                    res.get('Occupancy', -1), res.get('ScratchSize', -1), res.get('LDSByteSize', -1)))
        print('| | **all** | %d | %d | | | | |' % (tl, tw))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rev', default=None, help='git revision whose sources are compiled (default: the working tree)')
    ap.add_argument('--keep', default=None, help='directory that receives the assembly listings')
    a = ap.parse_args()
    report(a.rev, a.keep)
