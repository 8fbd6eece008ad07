"""CPU: the cross-compiled listing of csrc/invpref_truth_rank.hip -- every instance of the two templated kernels
(csrc/truth_rank_body.hpp) exists, runs on the matrix cores, and uses no more scratch memory than the per-form kernels they
replaced: none, except the two plain scans at four 64-float chunks, which spilled 84 bytes (float4 staging) and 104 bytes
(element-wise staging) before."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from invpref_kdd_2022_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_regs  # noqa: E402

# scratch bytes allowed per instance `kernel<DC, VEC, FORM>`; every other instance: 0
SPILLS = {'truth_scan_kernel<4, true, 0>': 84, 'truth_scan_kernel<4, false, 0>': 104}


@pytest.fixture(scope='module')
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'invpref_truth_rank_dev.s')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + [f for f in build.FLAGS if f != '-Wall'] +
                              ['--cuda-device-only', '-S', os.path.join(build.CSRC, 'invpref_truth_rank.hip'), '-o', out],
                              stderr=subprocess.DEVNULL)
        return kernel_regs.listing(out)


def test_every_instance_is_there_on_the_matrix_cores_within_its_scratch(listing):
    ks = kernel_regs.kernels(listing)
    scans = {k['name']: k for k in ks if k['name'].startswith('truth_scan_kernel')}
    keys = {k['name']: k for k in ks if k['name'].startswith('truth_key_kernel')}
    assert set(scans) == {'truth_scan_kernel<%d, %s, %d>' % (dc, vec, form)
                          for dc in (1, 2, 4) for vec in ('true', 'false') for form in (0, 1, 2)}
    assert set(keys) == {'truth_key_kernel<%d, %d>' % (dc, form) for dc in (1, 2, 4) for form in (0, 1, 2)}
    assert len(scans) == 18 and len(keys) == 9 and set(SPILLS) <= set(scans)
    for k in ks:                                                  # (the matrix route and the metric kernels too)
        assert k['scratch'] <= SPILLS.get(k['name'], 0), k
        if k['scratch'] == 0:
            assert k['scratch_ops'] == 0, k
    bodies = re.findall(r'\n(_Z\w*truth_(?:scan|key)_kernel\w*):(.*?)\.Lfunc_end', listing, re.S)
    assert len(bodies) == 27
    for name, body in bodies:
        assert 'v_mfma_f32_16x16x4_f32' in body, name
