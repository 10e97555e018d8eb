"""The gfx950 code objects inside the built library, read without a GPU and without recompiling (llvm-objdump --offloading
+ llvm-readelf --notes): the resource notes of every kernel, for the budget tests."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, '3d-fm-gan_amd', 'csrc', 'libfmgan_hip.so')
LLVM = '/opt/rocm/lib/llvm/bin'
NOTES = {'vgpr': r'\.vgpr_count', 'vgpr_spill': r'\.vgpr_spill_count', 'sgpr_spill': r'\.sgpr_spill_count',
         'scratch': r'\.private_segment_fixed_size', 'lds': r'\.group_segment_fixed_size'}


def kernel_notes(workdir):
    """{kernel name: {'vgpr', 'vgpr_spill', 'sgpr_spill', 'scratch', 'lds'}} of libfmgan_hip.so (built first if a fresh
    checkout has none), unpacked into `workdir`; skips the calling test when the LLVM tools are missing."""
    objdump, readelf = os.path.join(LLVM, 'llvm-objdump'), os.path.join(LLVM, 'llvm-readelf')
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip('llvm-objdump / llvm-readelf not found')
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    shutil.copy(LIB, workdir / 'lib.so')
    subprocess.run([objdump, '--offloading', str(workdir / 'lib.so')], check=True, capture_output=True, cwd=workdir)
    out = {}
    for f in sorted(os.listdir(workdir)):
        if not f.endswith('gfx950'):
            continue
        notes = subprocess.run([readelf, '--notes', str(workdir / f)], check=True, capture_output=True, text=True).stdout
        for blk in notes.split('- .agpr_count')[1:]:
            name = re.search(r'\.name:\s+(\S+)', blk).group(1)
            out[name] = {k: int(re.search(key + r':\s+(\d+)', blk).group(1)) for k, key in NOTES.items()}
    return out
