#!/usr/bin/env python3
"""Compare the device code of two trees kernel by kernel (CPU only; text comparison, runs nothing).

Usage: python tools/kernel_diff.py A B [--keep DIR] [--jobs N]

A and B are each either a source tree (has cubecobrarecommender_amd/csrc) or a directory of
device assembly (*.s, one per csrc/*.hip). A tree is compiled device-only with the product's
flags (build.py: -O3 -std=c++17, the file's FILE_FLAGS) into a temporary directory, or DIR/a and
DIR/b with --keep. Per kernel symbol the function body and its .amdhsa_kernel block (VGPRs, SGPRs,
LDS, scratch) are compared; only the compiler's local label numbering is normalised. Prints
identical / changed / removed / added per kernel and a summary; exit status 1 if anything changed.
"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ARCH = os.environ.get('CCREC_ARCH', 'gfx950')
FILE_FLAGS = {'decout.hip': ['-fno-honor-nans'], 'decreg.hip': ['-fno-honor-nans']}   # = build.py
LABEL = re.compile(r'\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI|LCPI)\d+(_?)')


def compile_tree(tree, out, jobs):
    csrc = os.path.join(tree, 'cubecobrarecommender_amd', 'csrc')
    inc = os.path.join(tree, 'include')
    os.makedirs(out, exist_ok=True)

    def one(f):
        cmd = [HIPCC, '-S', '--cuda-device-only', '-O3', '-std=c++17', f'--offload-arch={ARCH}',
               '-I', inc, '-I', csrc, *FILE_FLAGS.get(f, []), os.path.join(csrc, f),
               '-o', os.path.join(out, f[:-4] + '.s')]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'hipcc failed for {f}:\n{r.stderr}')

    with cf.ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, sorted(f for f in os.listdir(csrc) if f.endswith('.hip'))))
    return out


def kernels(asm_dir):
    """{(file, symbol): normalised text of the function body + its .amdhsa_kernel block}"""
    out = {}
    for f in sorted(os.listdir(asm_dir)):
        if not f.endswith('.s'):
            continue
        lines = open(os.path.join(asm_dir, f)).read().split('\n')
        body, desc, cur = {}, {}, None
        funcs = {m.group(1) for ln in lines for m in [re.match(r'\s*\.type\s+(\S+),@function', ln)] if m}
        for ln in lines:
            s = ln.strip()
            m = re.match(r'\.amdhsa_kernel\s+(\S+)', s)
            if m:
                cur = ('d', m.group(1))
                desc[cur[1]] = []
            elif s == '.end_amdhsa_kernel':
                cur = None
            elif cur and cur[0] == 'd':
                desc[cur[1]].append(s)
            elif s.endswith(':') and s[:-1] in funcs:
                cur = ('b', s[:-1])
                body[cur[1]] = []
            elif cur and cur[0] == 'b':
                if s.startswith('.Lfunc_end'):
                    cur = None
                elif s and not s.startswith(';'):
                    body[cur[1]].append(LABEL.sub(r'.\1N\2', s.split(' ;')[0].rstrip()))
        for k in funcs | set(desc):    # kernels, and any device function left out of line
            out[(f[:-2], k)] = '\n'.join(body.get(k, ['<no body>']) + ['--'] + desc.get(k, []))
    return out


def demangle(names):
    try:
        r = subprocess.run(['c++filt'], input='\n'.join(names),
                           capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split('\n')))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--keep', help='keep the compiled assembly under DIR/a and DIR/b')
    ap.add_argument('--jobs', type=int, default=8)
    ap.add_argument('--quiet', action='store_true', help='do not list identical kernels')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base = args.keep or tmp
        dirs = []
        for tag, p in (('a', args.a), ('b', args.b)):
            is_tree = os.path.isdir(os.path.join(p, 'cubecobrarecommender_amd', 'csrc'))
            dirs.append(compile_tree(p, os.path.join(base, tag), args.jobs) if is_tree else p)
        ka, kb = kernels(dirs[0]), kernels(dirs[1])
    names = demangle(sorted({k[1] for k in ka} | {k[1] for k in kb}))
    groups = {'identical': [], 'changed': [], 'removed': [], 'added': []}
    for k in sorted(set(ka) | set(kb)):
        g = 'added' if k not in ka else 'removed' if k not in kb else \
            'identical' if ka[k] == kb[k] else 'changed'
        groups[g].append(k)
    for g in ('identical', 'changed', 'removed', 'added'):
        if g == 'identical' and args.quiet:
            continue
        for f, sym in groups[g]:
            print(f'{g:9s} {f}: {names[sym]}')
    print('summary: ' + ', '.join(f'{len(v)} {g}' for g, v in groups.items()))
    return 1 if groups['changed'] else 0


if __name__ == '__main__':
    sys.exit(main())
