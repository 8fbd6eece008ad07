#!/usr/bin/env python3
"""tools/device_diff.py OLD_TREE NEW_TREE -- is the device program of two checkouts the same?

Every translation unit of build.SOURCES is compiled in both trees with build.FLAGS + `--cuda-device-only -S`, and the two
listings are compared as TEXT: `identical` (line for line, the lines naming the source-derived __hip_cuid_ symbol dropped),
`identical after reordering` (the same set of kernels, each with an equal body and descriptor once the function index in
local labels is normalised), or the first kernel that differs.  Exit status 1 on any difference.  A host-side refactor must
come out `identical`: the proof, without a GPU, that what the GPU executes has not changed."""
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
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
