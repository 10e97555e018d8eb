#!/usr/bin/env python3
"""Generate tests/golden/dataset.npz from the reference's dataset.py, imported on the CPU.

    FMGAN_REFERENCE=<checkout of adobe/3D-FM-GAN> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dataset.py

Run where the reference exists (not on the GPU box).  Under torch 2.10 `from torch.utils.data.sampler import Optional`
fails, so that one name is supplied first (torch.utils.data.sampler.Optional = typing.Optional); nothing else of the
reference is stubbed.  Recorded, over tests/dataset_cases.py's seeds and folder tree (written into a temporary folder):
    sampler/<dual|extreme>/<len>        the index sequence of one seeded epoch;  .../len: len(sampler)
    files/<dataset>/<list>              the file lists, relative to the tree's root, in the class's order
    items/<dataset>/<i>/<k>             image k of item i with transform=None, as a uint8 array
No reference source text is stored.
"""
import importlib.util
import os
import sys
import tempfile
import typing

import numpy as np
import torch
import torch.utils.data.sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dataset_cases as C  # noqa: E402


def reference_dataset_module():
    ref = os.environ.get('FMGAN_REFERENCE') or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref:
        raise SystemExit('set FMGAN_REFERENCE (or pass the path) to a checkout of the reference')
    torch.utils.data.sampler.Optional = typing.Optional
    spec = importlib.util.spec_from_file_location('reference_dataset', os.path.join(ref, 'dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(mod):
    out = {}
    for n in C.SAMPLER_LENS:
        for name, cls in (('dual', mod.DualSupervisionSampler), ('extreme', mod.ExtremePoseDualSupervisionSampler)):
            np_seed, torch_seed = C.SAMPLER_SEED[n]
            np.random.seed(np_seed)
            gen = torch.Generator()
            gen.manual_seed(torch_seed)
            s = cls(C.Sized(n), C.N_IMG_PER_ID, generator=gen)
            out[f'sampler/{name}/{n}'] = np.asarray(list(s), dtype=np.int64)
            out[f'sampler/{name}/{n}/len'] = np.int64(len(s))
    with tempfile.TemporaryDirectory() as root:
        dirs = C.write_tree(root)
        for name, ds in C.build_datasets(mod, dirs).items():
            for key, paths in C.file_lists(ds).items():
                out[f'files/{name}/{key}'] = np.asarray(C.relative(paths, root) if key != 'ids' else paths)
            out[f'files/{name}/len'] = np.int64(len(ds))
            if name == 'editing_train':
                np.random.seed(C.EDIT_TRAIN_SEED)
            for i in range(len(ds)):
                for k, a in enumerate(C.item_arrays(ds[i])):
                    out[f'items/{name}/{i}/{k}'] = a
    return out


if __name__ == '__main__':
    out = record(reference_dataset_module())
    path = os.path.join(ROOT, 'tests', 'golden', 'dataset.npz')
    np.savez_compressed(path, **out)
    print(path, len(out), os.path.getsize(path))
