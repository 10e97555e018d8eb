"""Register / spill budgets of the kernels the measured occupancies rely on, read from the code objects inside the built
library (tests/codeobj.py: llvm-objdump --offloading + llvm-readelf --notes, no GPU, no recompilation).

DESIGN §3.1 / §3.3 quote blocks per CU per tile (2 / 3 / 4 for the 128- / 64- / 32-channel modulated-conv tiles, 16 waves per
CU for the DMA-ring blur); those follow from `512 / vgpr_count` waves per SIMD.  A compiler or source change that pushes a
kernel over its budget, or makes it spill, silently costs a block per CU — this test makes it loud.
"""
import pytest

import codeobj


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    out = codeobj.kernel_notes(tmp_path_factory.mktemp('codeobj'))
    assert len(out) > 80, f'only {len(out)} kernels found in the library'
    return out


def _one(kernels, needle):
    hits = [k for k in kernels if needle in k]
    assert len(hits) == 1, (needle, hits)
    return kernels[hits[0]]


# (mangled-name fragment, max registers for the quoted blocks per CU = 512 // blocks, spills allowed)
MODCONV = [
    ('modconv_mfma_f32INS_18Plain128x256DmaKc4ELb0E', 256, False),   # 128 x 256 plain tile: 2 blocks per CU
    ('modconv_mfma_f32INS_17Plain64x256DmaKc4ELb0E', 170, False),   # 64 x 256 plain tile: 3
    ('modconv_mfma_f32INS_21Plain32x256DmaKc4R128ELb0E', 128, False),   # 32 x 256 plain tile, 4-channel chunks: 4
    ('modconv_mfma_f32INS_21Plain32x256DmaKc4R128ELb1E', 128, True),    # the same with the ToRGB epilogue (epilogue-only spills)
    ('modconv_mfma_f32INS_19Transposed64x128DmaELb0E', 256, False),   # transposed 64-channel tile: 2
    ('modconv_mfma_f32INS_23Transposed32x128DmaR128ELb0E', 128, True),    # transposed 32-channel tile: 4 (7 dwords in the epilogue)
]


@pytest.mark.parametrize('needle,budget,spills_ok', MODCONV, ids=[m[0][16:] for m in MODCONV])
def test_modconv_tiles_fit_their_blocks_per_cu(kernels, needle, budget, spills_ok):
    k = _one(kernels, needle)
    assert k['vgpr'] <= budget, k
    if not spills_ok:
        assert k['vgpr_spill'] == 0 and k['scratch'] == 0, k
    else:
        assert k['vgpr_spill'] <= 32, k


def test_reduced_precision_and_split_operand_kernels_do_not_spill(kernels):
    names = [k for k in kernels if 'modconv_mfma_bf16' in k]
    assert len(names) == 8, names                      # 6 bf16 instantiations + 2 split-operand ones
    for n in names:
        assert kernels[n]['vgpr_spill'] == 0 and kernels[n]['scratch'] == 0 and kernels[n]['vgpr'] <= 256, (n, kernels[n])


def test_streaming_kernels_keep_their_occupancy(kernels):
    # DMA-ring blur with the fused epilogue: 64 registers = 8 waves per SIMD (its ring lives in LDS, not in registers)
    k = _one(kernels, 'ufd_dmaring_f32ILb1ELb0ELb0E')
    assert k['vgpr'] <= 64 and k['vgpr_spill'] == 0 and k['scratch'] == 0, k
    for needle, budget in (('ufd_rowmarch_f32ILi4ELb1E', 128), ('noise_bias_act_f32', 32), ('equal_linear_f32', 32),
                           ('modconv_demod_f32ILb1E', 40), ('fba_f32_inner4ILi30ELb0E', 32)):
        k = _one(kernels, needle)
        assert k['vgpr'] <= budget and k['vgpr_spill'] == 0 and k['scratch'] == 0, (needle, k)
