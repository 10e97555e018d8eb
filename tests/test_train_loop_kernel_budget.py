"""The two kernels of the training loop (csrc/train_loop.hip) in the built library's gfx950 code object, read without a
GPU (tests/codeobj.py): each is there exactly once; neither spills, uses scratch memory or LDS.  train_loss_row's 16
pointers arrive by value and must be picked in place (16 uniform selects), not copied to scratch and indexed by lane.
"""
import pytest

import codeobj

KERNELS = ('train_ema_f32', 'train_loss_row_f32')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    notes = codeobj.kernel_notes(tmp_path_factory.mktemp('codeobj'))
    return {name: k for name, k in notes.items() if 'train_ema' in name or 'train_loss_row' in name}


def test_each_kernel_is_built_once(kernels):
    for want in KERNELS:
        assert sum(want in name for name in kernels) == 1, (want, sorted(kernels))
    assert len(kernels) == len(KERNELS), sorted(kernels)


def test_no_spills_no_scratch_no_lds(kernels):
    assert kernels
    for name, k in sorted(kernels.items()):
        print(name, k)
        assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0 and k['lds'] == 0, (name, k)
        assert k['vgpr'] <= 128, (name, k)          # 512 / 128: a SIMD still holds four waves (the bound of the L-BFGS kernels)
