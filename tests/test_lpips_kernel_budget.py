"""Register budget of the LPIPS-distance kernels (csrc/lpips_distance.hip), read from the code objects inside the built
library the way tests/test_kernel_budgets.py does (tests/codeobj.py: no GPU).

The kernels hold both features of a pixel and the 1x1 weight in registers (96 payload registers at C = 512) and are
launched at 8 blocks of 4 waves per CU for the narrow taps, 4 for the wide ones: 128 registers is the budget of four waves
per SIMD, and a spill would put feature-sized traffic back into memory — the traffic the kernels exist to remove.
"""
import pytest

import codeobj


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    notes = codeobj.kernel_notes(tmp_path_factory.mktemp('codeobj'))
    return {name: k for name, k in notes.items() if 'lpips_dist' in name}


def test_every_instantiation_is_built(kernels):
    """Forward: one per channel count; backward: per channel count, grad_f1 only / grad_f0 only / both."""
    fwd = [k for k in kernels if 'lpips_dist_fwd_f32' in k]
    bwd = [k for k in kernels if 'lpips_dist_bwd_f32' in k]
    assert len(fwd) == 4 and len(bwd) == 12 and len(kernels) == 16, sorted(kernels)
    for c in (64, 128, 256, 512):
        assert sum(f'ILi{c}E' in k for k in fwd) == 1 and sum(f'ILi{c}E' in k for k in bwd) == 3, c


def test_no_spills_no_scratch_at_most_128_registers(kernels):
    assert kernels
    for name, k in sorted(kernels.items()):
        print(name, k)
        assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0, (name, k)
        assert k['vgpr'] <= 128, (name, k)
