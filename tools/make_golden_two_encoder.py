#!/usr/bin/env python3
"""Generate tests/golden/two_encoder.npz: the reference's 2-encoder scheme (Forward_Inference) on the CPU.

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_two_encoder.py
The reference is imported exactly as tools/make_golden.py imports it (JIT and torchvision stubbed; importing that
module does it).  Cases, builders and weights come from tests/two_encoder_cases.py on both sides; the file holds OUTPUTS
only.  Per forward case: the strided sample of the [B,3,S,S] image (`/sub`), the whole-image statistics (`/stats`) and
the float64 run's sample (`/sub64`).  Per re-animation case the same, from the reference run frame by frame with the
one photo (its GIF driver's loop).  The gradient case: image sample, L1 loss, and a strided sample + norm of every
parameter gradient of the three modules, in fp32 and float64 (make_golden._sample_grads).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (stubs the JIT, puts the reference and tests/ on sys.path)
import two_encoder_cases as tc  # noqa: E402


def build(c, dt):
    mods = tc.build(c, mg.resnet_encoder, mg.psp_encoders, mg.stylegan2)
    for m in mods:
        m.to(dt)
    return mods


def forward(c, p, r, mods):
    e_tsr, e_w, g = mods
    return mg.network_util.Forward_Inference(p, r, e_tsr, e_w, mg._GWrap(g), mod_encode=c['mod_encode'],
                                             co_modulation=c['co_mod'], sliced_layer=c['sliced_layer'],
                                             use_tanh=c['use_tanh'])


def run_forward(c, dt):
    p, r = (t.to(dt) for t in tc.inputs(c))
    return forward(c, p, r, build(c, dt))


def run_reanimate(c, dt):
    p, r = (t.to(dt) for t in tc.reanimate_inputs(c))
    mods = build(c, dt)
    return torch.cat([forward(c, p, r[t:t + 1], mods) for t in range(c['frames'])], 0)


def gen_grad(out):
    c = tc.GRAD_CASE
    for dt, sfx in ((torch.float32, ''), (torch.float64, '64')):
        e_tsr, e_w, g = build(c, dt)
        p, r = (t.to(dt) for t in tc.inputs(c))
        img = forward(c, p, r, (e_tsr, e_w, g))
        loss = mg.ref_training_util.L1_Loss(img, tc.target(c).to(dt))
        loss.backward()
        out['grad/img/sub' + sfx] = mg.subsample(img, c['stride'])
        out['grad/loss' + sfx] = np.float64(loss.item())
        for k, m in (('e_tsr', e_tsr), ('e_w', e_w), ('g', g)):
            mg._sample_grads(out, 'grad/' + k, m.named_parameters(), sfx)
        print('  grad', dt, loss.item(), float(img.abs().max()), flush=True)


def main():
    out = {}
    with torch.no_grad():
        for cases_, run in ((tc.FORWARD_CASES, run_forward), (tc.REANIMATE_CASES, run_reanimate)):
            for c in cases_:
                img = run(c, torch.float32)
                assert tuple(img.shape) == (c.get('b', c.get('frames')), 3, c['size'], c['size'])
                out[c['name'] + '/sub'] = mg.subsample(img, c['stride'])
                out[c['name'] + '/stats'] = mg.stats(img)
                out[c['name'] + '/sub64'] = mg.subsample(run(c, torch.float64), c['stride'])
                print(' ', c['name'], tuple(img.shape), float(img.abs().max()), flush=True)
    gen_grad(out)
    np.savez_compressed(os.path.join(mg.OUT, 'two_encoder.npz'), **out)
    print('two_encoder', len(out))


if __name__ == '__main__':
    main()
