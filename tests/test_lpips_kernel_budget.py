"""Register budget of the LPIPS-distance kernels (csrc/lpips_distance.hip), read from the code objects inside the built
library the way tests/test_kernel_budgets.py does (llvm-objdump --offloading + llvm-readelf --notes: no GPU).

The kernels hold both features of a pixel and the 1x1 weight in registers (96 payload registers at C = 512) and are
launched at 8 blocks of 4 waves per CU for the narrow taps, 4 for the wide ones: 128 registers is the budget of four waves
per SIMD, and a spill would put feature-sized traffic back into memory — the traffic the kernels exist to remove.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, '3d-fm-gan_amd', 'csrc', 'libfmgan_hip.so')
LLVM = '/opt/rocm/lib/llvm/bin'


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    objdump, readelf = os.path.join(LLVM, 'llvm-objdump'), os.path.join(LLVM, 'llvm-readelf')
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip('llvm-objdump / llvm-readelf not found')
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    d = tmp_path_factory.mktemp('codeobj')
    shutil.copy(LIB, d / 'lib.so')
    subprocess.run([objdump, '--offloading', str(d / 'lib.so')], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if not f.endswith('gfx950'):
            continue
        notes = subprocess.run([readelf, '--notes', str(d / f)], check=True, capture_output=True, text=True).stdout
        for blk in notes.split('- .agpr_count')[1:]:
            name = re.search(r'\.name:\s+(\S+)', blk).group(1)
            if 'lpips_dist' not in name:
                continue

            def num(key):
                return int(re.search(key + r':\s+(\d+)', blk).group(1))
            out[name] = {'vgpr': num(r'\.vgpr_count'), 'vgpr_spill': num(r'\.vgpr_spill_count'),
                         'sgpr_spill': num(r'\.sgpr_spill_count'), 'scratch': num(r'\.private_segment_fixed_size')}
    return out


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
