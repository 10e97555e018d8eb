#!/usr/bin/env python3
"""Generate tests/golden/fid.npz: Frechet Inception distances by the reference's own calc_fid and
extract_feature_from_samples on CPU, for the cases of tests/fid_cases.py.

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_fid.py
The reference is imported exactly as tools/make_golden.py imports it (JIT and torchvision stubbed; importing that module
does it); scipy is the real one.  Evaluation/fid.py pulls in calc_inception.py and inception.py, which subclass
torchvision's Inception blocks at import: the stub gets `transforms`, `models` (with `inception.InceptionA/C/E` as empty
classes) and `models.utils`; `tqdm` is stubbed when absent.  None of those is used: the Inception network of the sample
cases is fid_cases.StandinInception on both sides.  The module's `torch` is replaced for the sample cases by a proxy whose
randn returns the case's latents (tools/make_golden_ppl.py does the same).

The file holds OUTPUTS only, all scalars: per case `/fid`, `/spread_sym`, `/spread_mean` (tests/fid_cases.py).  For the
rank-deficient case the tool asserts that the reference's matrix square root is finite and that the imaginary part of its
diagonal is far under the reference's own 1e-3 gate.
"""
import os
import sys
import types

import numpy as np
import torch
from scipy import linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (stubs the JIT, puts the reference and tests/ on sys.path)
import fid_cases as fc  # noqa: E402

_tv = sys.modules['torchvision']
_tv.transforms = types.ModuleType('torchvision.transforms')
_tv.models = types.ModuleType('torchvision.models')
_tv.models.inception_v3 = _tv.models.Inception3 = type('Inception3', (torch.nn.Module,), {})
_tv.models.inception = types.ModuleType('torchvision.models.inception')
for _n in ('InceptionA', 'InceptionC', 'InceptionE'):
    setattr(_tv.models.inception, _n, type(_n, (torch.nn.Module,), {}))
_tv.models.utils = types.ModuleType('torchvision.models.utils')
_tv.models.utils.load_state_dict_from_url = None
for _m in ('transforms', 'models', 'models.inception', 'models.utils'):
    _mod = _tv
    for _part in _m.split('.'):
        _mod = getattr(_mod, _part)
    sys.modules['torchvision.' + _m] = _mod
try:
    import tqdm  # noqa: F401
except ImportError:
    _tq = types.ModuleType('tqdm'); _tq.tqdm = lambda it, *a, **k: it
    sys.modules['tqdm'] = _tq
from Evaluation import fid as ref_fid  # noqa: E402


def spreads(mean_a, cov_a, mean_b, cov_b, feat_a, feat_b):
    """(fid, spread_sym, spread_mean) of the reference for one pair of moments; feat_*: the fp32 features, for the
    float64 means."""
    fid = ref_fid.calc_fid(mean_a, cov_a, mean_b, cov_b)
    back = ref_fid.calc_fid(mean_b, cov_b, mean_a, cov_a)
    m64 = ref_fid.calc_fid(np.mean(feat_a.astype(np.float64), 0), cov_a,
                           mean_b if feat_b is None else np.mean(feat_b.astype(np.float64), 0), cov_b)
    return np.float64(fid), np.float64(abs(fid - back)), np.float64(abs(fid - m64))


def calc_case(name, d, n1, n2):
    fa, fb = fc.features(name, 'a', n1, d), fc.features(name, 'b', n2, d)
    assert fa.dtype == np.float32 and fa.mean() > 0.1
    (ma, ca), (mb, cb) = fc.moments(fa), fc.moments(fb)
    assert ma.dtype == np.float32 and ca.dtype == np.float64
    root, _ = linalg.sqrtm(ca @ cb, disp=False)
    imag = float(np.abs(np.diagonal(root).imag).max()) if np.iscomplexobj(root) else 0.0
    rank = int(np.linalg.matrix_rank(ca))
    print(f'  {name}: rank {rank} of {d}, sqrtm finite {bool(np.isfinite(root).all())}, max |imag diag| {imag:.3e}')
    assert np.isfinite(root).all() and imag < 1e-5, f'{name}: the reference would take its eps branch or raise'
    if name == 'rank':
        assert rank < d
    return spreads(ma, ca, mb, cb, fa, fb)


class _Torch:
    """Stands in for torch inside the reference module: randn hands out the case's latents, batch by batch."""

    def __init__(self, c):
        self.c, self.batch = c, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def randn(self, batch, dim, device=None):
        assert dim == 512
        z = fc.latents(self.c, self.batch, batch)
        self.batch += 1
        return z


def sample_case(c):
    if c['kind'] == 'toy':
        g = fc.ToyGenerator()
    else:
        g = mg.stylegan2.Generator(c['size'], 512, 8)
        g.load_state_dict(mg.synth.state_dict('generator', g.state_dict(), seed=4))
        g = fc.Pinned(g)
    saved = ref_fid.torch
    try:
        ref_fid.torch = proxy = _Torch(c)
        feat = ref_fid.extract_feature_from_samples(g, fc.StandinInception(), 1, None, c['batch'], c['n_sample'], 'cpu')
    finally:
        ref_fid.torch = saved
    feat = feat.numpy()
    assert feat.shape == (c['n_sample'], fc.FEATURES) and proxy.batch == 2 and feat.dtype == np.float32
    real = fc.real_stats()
    mean, cov = fc.moments(feat)
    return spreads(mean, cov, real['mean'], real['cov'], feat, None)


def main():
    out = {}
    with torch.no_grad():
        for name, d, n1, n2 in fc.CALC_CASES:
            res = calc_case(name, d, n1, n2)
            out[name + '/fid'], out[name + '/spread_sym'], out[name + '/spread_mean'] = res
            print(' ', name, 'fid', res[0], 'spread_sym', res[1], 'spread_mean', res[2], flush=True)
        for c in fc.SAMPLE_CASES:
            res = sample_case(c)
            n = 'sample_' + c['name']
            out[n + '/fid'], out[n + '/spread_sym'], out[n + '/spread_mean'] = res
            print(' ', n, 'fid', res[0], 'spread_sym', res[1], 'spread_mean', res[2], flush=True)
    np.savez_compressed(os.path.join(mg.OUT, 'fid.npz'), **out)
    print('fid', len(out))


if __name__ == '__main__':
    main()
