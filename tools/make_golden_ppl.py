#!/usr/bin/env python3
"""Generate tests/golden/ppl.npz: perceptual path lengths by the reference's own Get_PPL_Score on CPU.

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ppl.py
The reference is imported exactly as tools/make_golden.py imports it (JIT and torchvision stubbed; importing that module
does it).  Evaluation/ppl.py needs three more substitutions:
  * `model` (a module the reference does not ship; only the script half uses its Generator) and `lpips` (not importable
    offline) are stubbed in sys.modules.  The stub's PerceptualLoss(...) hands out a recorder round the case's distance:
    the stand-in ((x - y)^2).mean([1, 2, 3]) for `toy`, the project's lpips.PerceptualLoss with the weights of
    ppl_cases.percept_state_dict for the Generator cases (loaded from its file under another name, with op.lpips_distance
    stubbed: `op` is the reference's package in this process, and on CPU tensors the module takes its aten composite);
  * the module's `torch` is replaced for the call by a proxy whose randn / rand return the case's synth tensors
    (tools/make_golden_quant_eval.py replaces `np` the same way), and its `np` by one whose percentile accepts
    `interpolation=` on a numpy that has dropped it;
  * the Generator sits behind a wrapper with `.module` that pins the stored noise, records latent_e and, for the crop
    case, crops the image as the reference's script half does before the function's own reduction.
Each case runs in fp32 and in float64.  Inputs and weights come from tests/synth.py on both sides; the file holds OUTPUTS
only: per case `/dist`, `/score` (fp32 run), `/dist64`, `/score64` and `/latent_e64` (first batch).
The two conditions of tests/ppl_cases.py on eps are asserted here.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (stubs the JIT, puts the reference and tests/ on sys.path)
import ppl_cases as pc  # noqa: E402

_model = types.ModuleType('model'); _model.Generator = None
sys.modules['model'] = _model
_lpips = types.ModuleType('lpips'); _lpips.PerceptualLoss = None
sys.modules['lpips'] = _lpips
from Evaluation import ppl as ref_ppl  # noqa: E402


def project_lpips():
    """The project's lpips module, loaded from its file as `fmgan_lpips`."""
    stub = types.ModuleType('op.lpips_distance')
    stub.lpips_distance, stub.lpips_distance_serves = None, (lambda *a, **k: False)
    sys.modules['op.lpips_distance'] = stub
    path = os.path.join(mg.ROOT, '3d-fm-gan_amd', 'lpips', '__init__.py')
    spec = importlib.util.spec_from_file_location('fmgan_lpips', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Torch:
    """Stands in for torch inside the reference module: randn / rand hand out the case's samples, batch by batch."""

    def __init__(self, c, dt):
        self.c, self.dt, self.batch = c, dt, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def randn(self, shape, device=None):
        z = pc.inputs(self.c, self.batch)[0].to(self.dt)
        assert list(shape) == list(z.shape)
        return z

    def rand(self, n, device=None):
        t = pc.inputs(self.c, self.batch)[1].to(self.dt)
        assert n == t.shape[0]
        self.batch += 1
        return t


class _Numpy:
    """Stands in for numpy inside the reference module: percentile(interpolation=) also on a numpy that refuses it."""

    def __getattr__(self, name):
        return getattr(np, name)

    def percentile(self, a, q, interpolation='linear'):
        try:
            return np.percentile(a, q, interpolation=interpolation)
        except TypeError:
            return np.percentile(a, q, method=interpolation)


class _Pinned(nn.Module):
    """The generator as Get_PPL_Score wants it (`module.` in the state_dict keys), with the stored noise pinned."""

    def __init__(self, g, crop):
        super().__init__()
        self.module, self.crop, self.latents = g, crop, []

    def forward(self, **kw):
        self.latents.append(kw['latent_styles'][0].clone())
        image = self.module(randomize_noise=False, **kw)
        if self.crop:
            c = image.shape[2] // 8
            image = image[:, :, c * 3:c * 7, c * 2:c * 6]
        return image


class _Recorded:
    """What the stubbed lpips.PerceptualLoss(...) returns: the case's distance, keeping every batch's values."""

    def __init__(self, distance):
        self.distance, self.values = distance, []

    def __call__(self, pred, target):
        d = self.distance(pred, target)
        self.values.append(d.reshape(-1).clone())
        return d


def run(c, dt, lp):
    if c['kind'] == 'toy':
        g, distance = pc.ToyGenerator(c['latent_dim']), pc.standin_distance
    else:
        g = mg.stylegan2.Generator(c['size'], 512, 8)
        g.load_state_dict(mg.synth.state_dict('generator', g.state_dict(), seed=4))
        distance = lp.PerceptualLoss(model='net-lin', net='vgg')
        distance.load_state_dict(pc.percept_state_dict(distance.state_dict()))
        distance = distance.to(dt)
    wrap = _Pinned(g.to(dt).eval(), c['crop'])
    rec = _Recorded(distance)
    saved = ref_ppl.torch, ref_ppl.np
    try:
        ref_ppl.torch, ref_ppl.np = _Torch(c, dt), _Numpy()
        _lpips.PerceptualLoss = lambda **kw: rec
        score = ref_ppl.Get_PPL_Score(wrap, c['n_sample'], c['batch'], c['eps'], c['latent_dim'], 'cpu', [0])
    finally:
        ref_ppl.torch, ref_ppl.np = saved
    dist = torch.cat(rec.values).double().numpy()
    assert dist.shape == (c['n_sample'] // c['batch'] * c['batch'],)
    return dict(dist=dist, score=np.float64(score), latent_e=wrap.latents[0].double().numpy())


def check(c, d32, d64):
    err = np.abs(d32 - d64).max()
    print(f"  {c['name']}: eps {c['eps']:g} max|dist32 - dist64| {err:.3e} median {np.median(d64):.3e} "
          f"min {d64.min():.3e} max {d64.max():.3e}", flush=True)
    assert err <= 1e-2 * np.median(d64), f"{c['name']}: condition (a) fails: raise eps tenfold in tests/ppl_cases.py"
    if c['kind'] == 'toy':
        s = np.sort(d64)
        lo, hi = int(np.floor(0.01 * (len(s) - 1))), int(np.ceil(0.99 * (len(s) - 1)))
        gaps = (s[lo] - s[lo - 1], s[hi + 1] - s[hi])
        print(f'  {c["name"]}: cuts after sorted index {lo - 1} and {hi}, gaps {gaps[0]:.3e} {gaps[1]:.3e}', flush=True)
        assert lo >= 1 and hi + 1 < len(s) and min(gaps) > 8 * err, \
            f"{c['name']}: condition (b) fails: raise eps tenfold in tests/ppl_cases.py"


def main():
    lp = project_lpips()
    out = {}
    with torch.no_grad():
        for c in pc.PPL_CASES:
            res = {dt: run(c, dt, lp) for dt in (torch.float32, torch.float64)}
            r32, r64 = res[torch.float32], res[torch.float64]
            check(c, r32['dist'], r64['dist'])
            n = c['name']
            out[n + '/dist'], out[n + '/score'] = r32['dist'], r32['score']
            out[n + '/dist64'], out[n + '/score64'] = r64['dist'], r64['score']
            out[n + '/latent_e64'] = r64['latent_e']
            print(' ', n, 'score', float(r32['score']), float(r64['score']), flush=True)
    np.savez_compressed(os.path.join(mg.OUT, 'ppl.npz'), **out)
    print('ppl', len(out))


if __name__ == '__main__':
    main()
