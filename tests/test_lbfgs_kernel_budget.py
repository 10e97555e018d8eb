"""The L-BFGS kernels (csrc/lbfgs.hip) in the built library's gfx950 code object, read without a GPU (tests/codeobj.py):
each of the five kernels of a fused step, and the one-block reduction two of them end with, is there exactly once, and none
spills or uses scratch memory.  lbfgs_pair keeps a tile of 8 elements per lane of s, y and g in registers while it walks
the history; its segment table arrives by value and must be indexed in place, not copied to scratch.
"""
import pytest

import codeobj

KERNELS = ('lbfgs_pair', 'lbfgs_coeffs', 'lbfgs_direction', 'lbfgs_update', 'lbfgs_gather', 'lbfgs_reduce')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    notes = codeobj.kernel_notes(tmp_path_factory.mktemp('codeobj'))
    return {name: k for name, k in notes.items() if 'lbfgs_' in name}


def test_each_kernel_is_built_once(kernels):
    for want in KERNELS:
        assert sum(want in name for name in kernels) == 1, (want, sorted(kernels))
    assert len(kernels) == len(KERNELS), sorted(kernels)


def test_no_spills_no_scratch(kernels):
    assert kernels
    for name, k in sorted(kernels.items()):
        print(name, k)
        assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0, (name, k)
        assert k['vgpr'] <= 128, (name, k)
    pair = next(k for name, k in kernels.items() if 'lbfgs_pair' in name)
    coeffs = next(k for name, k in kernels.items() if 'lbfgs_coeffs' in name)
    assert pair['lds'] == (6 * 32 + 7) * 4 * 8 and coeffs['lds'] <= 64 * 1024
