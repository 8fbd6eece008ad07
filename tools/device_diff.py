#!/usr/bin/env python3
"""tools/device_diff.py OLD_TREE NEW_TREE -- is the device program of two checkouts the same?

Every translation unit of build.SOURCES is compiled in both trees with build.FLAGS + `--cuda-device-only -S`, and the two
listings are compared as TEXT: `identical` (line for line, the lines naming the source-derived __hip_cuid_ symbol dropped),
`identical after reordering` (the same set of kernels, each with an equal body and descriptor once the function index in
local labels is normalised), or the first kernel that differs.  Exit status 1 on any difference.  A host-side refactor must
come out `identical`: the proof, without a GPU, that what the GPU executes has not changed.

tools/device_diff.py --kernels OLD_TREE NEW_TREE [OLD_NAME=NEW_NAME ...] [file.hip ...] -- the same comparison kernel by
kernel, for a change that is meant to move device code: for each translation unit (the named ones, or all) one line per kernel
of either tree with the verdict (`equal`, `differs`, `only old`, `only new`) and next_free_vgpr / accum_offset / scratch
bytes / LDS bytes of both sides.  Names are demangled.  OLD_NAME=NEW_NAME pairs renamed instances by prefix; a `*` on
both sides stands for the instance's own template arguments: 'scan_scaled_kernel<*>=scan_kernel<*, 1>'.  Always exits 0."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'invpref_kdd_2022_amd'))
import build  # noqa: E402  (SOURCES, FLAGS, _hipcc: the project's own)

CSRC = os.path.join('invpref_kdd_2022_amd', 'csrc')


def listing(tree, src, tmp, tag):
    out = os.path.join(tmp, tag + '_' + os.path.splitext(src)[0] + '.s')
    subprocess.check_call([build._hipcc()] + build.FLAGS + ['--cuda-device-only', '-S', os.path.join(tree, CSRC, src), '-o', out],
                          stderr=subprocess.DEVNULL)
    return [ln for ln in open(out).read().split('\n') if '__hip_cuid_' not in ln]


def kernels(lines):
    """{name: body + descriptor block}, the function index <n> of .LBB<n>_ / BB<n>_ / .Lfunc_end<n> normalised"""
    text = '\n'.join(lines)
    res = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', text, re.S):
        name = m.group(1)
        i = text.index('\n' + name + ':')
        j = re.compile(r'\.Lfunc_end\d+:').search(text, i).start()
        # (.LBB<n>_ labels, the BB<n>_ of block comments, and the comment column, which moves with the width of <n>)
        body = re.sub(r' +;', ' ;', re.sub(r'BB\d+_', 'BB#_', text[i:j]))
        res[name] = body + re.sub(r'\.Lfunc_end\d+', '.Lfunc_end#', m.group(2))
    return res


FIGURES = ('next_free_vgpr', 'accum_offset', 'private_segment_fixed_size', 'group_segment_fixed_size')


def short_names(names):
    """mangled -> `kernel<args>`: demangled, without the unnamed namespace, the return type and the parameter list"""
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return {n: re.sub(r'\(anonymous namespace\)::|^void |\(.*', '', d) for n, d in zip(names, dem)}


def kernel_rows(old, new, renames):
    """[(old short name or None, new short name or None, verdict, old figures, new figures)]"""
    sides = []
    for lines in (old, new):
        ks = kernels(lines)
        short = short_names(sorted(ks))
        # (a renamed instance names itself in labels and symbols: its own name is masked before bodies are compared)
        sides.append({short[n]: (b.replace(n, '@'), [int(re.search(r'\.amdhsa_%s\s+(\d+)' % f, b).group(1)) for f in FIGURES])
                      for n, b in ks.items()})
    ko, kn = sides
    rows, paired = [], set()
    for name in sorted(ko):
        to = name
        for a, b in renames:
            m = re.fullmatch(re.escape(a).replace(r'\*', '(.*)'), name)
            if m:
                to = b.replace('*', m.group(1))
        if to in kn:
            paired.add(to)
            rows.append((name, to, 'equal' if ko[name][0] == kn[to][0] else 'differs', ko[name][1], kn[to][1]))
        else:
            rows.append((name, None, 'only old', ko[name][1], None))
    rows += [(None, n, 'only new', None, kn[n][1]) for n in sorted(kn) if n not in paired]
    return rows


def main_kernels(old_tree, new_tree, rest):
    renames = []
    for a, b in (r.split('=', 1) for r in rest if '=' in r):
        renames.append((a, b) if '*' in a else (a + '*', b + '*'))
    sources = [r for r in rest if '=' not in r] or build.SOURCES
    fig = lambda f: '%3d %3d %4d %6d' % tuple(f) if f else '%17s' % '-'  # noqa: E731
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=16) as pool:
        jobs = [(src, pool.submit(listing, old_tree, src, tmp, 'old'), pool.submit(listing, new_tree, src, tmp, 'new'))
                for src in sources]
        for src, a, b in jobs:
            print('%s    (vgpr accum scratch lds: old | new)' % src)
            for o, n, verdict, fo, fn in kernel_rows(a.result(), b.result(), renames):
                print('  %-9s %s | %s  %s' % (verdict, fig(fo), fig(fn), o if n in (o, None) else (n if o is None else o + ' -> ' + n)))
    return 0


def compare(old, new):
    if old == new:
        return 'identical'
    ko, kn = kernels(old), kernels(new)
    for name in ko:
        if name in kn and ko[name] != kn[name]:
            return 'DIFFERENT: kernel %s' % name
    if set(ko) != set(kn):   # (a renamed kernel shows as one name on each side; their bodies are printed equal or not)
        gone, come = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
        strip = lambda n, b: b.replace(n, '@')  # noqa: E731
        same = len(gone) == len(come) == 1 and strip(gone[0], ko[gone[0]]) == strip(come[0], kn[come[0]])
        return 'DIFFERENT: only old %s, only new %s (%s); every other kernel equal' % (
            gone, come, 'one rename, equal bodies' if same else 'bodies differ')
    return 'identical after reordering'


def main(old_tree, new_tree):
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=16) as pool:
        jobs = [(src, pool.submit(listing, old_tree, src, tmp, 'old'), pool.submit(listing, new_tree, src, tmp, 'new'))
                for src in build.SOURCES]
        verdicts = [(src, compare(a.result(), b.result())) for src, a, b in jobs]
    for src, v in verdicts:
        print('%-24s %s' % (src, v))
    return int(any(v.startswith('DIFFERENT') for _, v in verdicts))


if __name__ == '__main__':
    if len(sys.argv) >= 4 and sys.argv[1] == '--kernels':
        sys.exit(main_kernels(sys.argv[2], sys.argv[3], sys.argv[4:]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
