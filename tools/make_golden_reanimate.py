#!/usr/bin/env python3
"""Generate tests/golden/reanimate.npz: one photo re-animated by a sequence of renders, by the reference on CPU.

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_reanimate.py
The reference is imported exactly as tools/make_golden.py imports it (JIT and torchvision stubbed; importing that
module does it).  Each case of tests/reanimate_cases.py runs the reference's own Forward_Inference_3_Encoder frame by
frame with the one photo, as its GIF driver does (Evaluation/visual_eval.py:174-184), in fp32 and in float64.  Inputs
and weights come from tests/synth.py on both sides; the file holds OUTPUTS only: per case the strided sample of the
[frames,3,S,S] images (`/sub`), the whole-image statistics (`/stats`) and the float64 run's sample (`/sub64`).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (stubs the JIT, puts the reference and tests/ on sys.path)
import reanimate_cases  # noqa: E402


def run(c, dt):
    n_latent = int(np.log2(c['size'])) * 2 - 2
    e_tsr, e_w, e_wp = mg.build_encoders(n_latent)
    g = mg.stylegan2.Generator(c['size'], 512, 8)
    g.load_state_dict(mg.synth.state_dict('generator', g.state_dict(), seed=4))
    g.eval()
    for m in (e_tsr, e_w, e_wp, g):
        m.to(dt)
    p, r = reanimate_cases.inputs(c)
    p, r = p.to(dt), r.to(dt)
    frames = [mg.network_util.Forward_Inference_3_Encoder(p, r[t:t + 1], e_tsr, e_w, e_wp, mg._GWrap(g),
                                                          tsr_encode=c['tsr_encode'], sliced_layer=c['sliced_layer'],
                                                          use_tanh=c['use_tanh']) for t in range(c['frames'])]
    return torch.cat(frames, 0)


def main():
    out = {}
    with torch.no_grad():
        for c in reanimate_cases.REANIMATE_CASES:
            img = run(c, torch.float32)
            assert tuple(img.shape) == (c['frames'], 3, c['size'], c['size'])
            out[c['name'] + '/sub'] = mg.subsample(img, c['stride'])
            out[c['name'] + '/stats'] = mg.stats(img)
            out[c['name'] + '/sub64'] = mg.subsample(run(c, torch.float64), c['stride'])
            print(' ', c['name'], tuple(img.shape), float(img.abs().max()), flush=True)
    np.savez_compressed(os.path.join(mg.OUT, 'reanimate.npz'), **out)
    print('reanimate', len(out))


if __name__ == '__main__':
    main()
