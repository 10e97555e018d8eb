"""Perceptual-path-length cases shared by tools/make_golden_ppl.py (reference side) and the tests.  Fixture:
tests/golden/ppl.npz, outputs only: per case the per-pair distances and the score of the reference's Get_PPL_Score in
fp32 (`/dist`, `/score`) and float64 (`/dist64`, `/score64`), and the first batch's interpolated latents (`/latent_e64`).

Samples come from tests/synth.py on both sides (`sampler`): noise_z is N(0,1), lerp_t is U(0,1).  The perceptual module of
the Generator cases is the project's lpips.PerceptualLoss on both sides with the weights of `percept_state_dict`; the toy
case uses a stand-in distance and a small generator that also runs on the CPU.

`eps` starts at 1e-2 (the reference's default 1e-4 makes the two images of a pair equal to within fp32 noise at these
weights) and is raised tenfold per case until the tool's two conditions hold:
  (a) max|dist32 - dist64| <= 1e-2 * median(dist64)
  (b) toy only: the gaps between the sorted distances either side of each percentile cut exceed 8 * max|dist32 - dist64|
"""
import torch
from torch import nn

import synth

PPL_CASES = [
    # 256 pairs: the percentile filter drops two values at each end
    dict(name='toy', kind='toy', latent_dim=16, n_sample=256, batch=64, eps=1e-2, crop=False),
    dict(name='g64', kind='generator', size=64, latent_dim=512, n_sample=8, batch=4, eps=1e-2, crop=False),
    dict(name='g512', kind='generator', size=512, latent_dim=512, n_sample=2, batch=2, eps=1e-2, crop=False),
    dict(name='g512_crop', kind='generator', size=512, latent_dim=512, n_sample=2, batch=2, eps=1e-2, crop=True),
]
BY_NAME = {c['name']: c for c in PPL_CASES}


def inputs(c, batch_index):
    """(noise_z [2B, D], lerp_t [B]) of one batch, fp32 on the CPU."""
    z = synth.tensor(f"ppl/{c['name']}/z/{batch_index}", (2 * c['batch'], c['latent_dim']))
    t = (synth.tensor(f"ppl/{c['name']}/t/{batch_index}", (c['batch'],), dist='uniform') + 1) / 2
    return z, t


def sampler(c, dtype=torch.float32):
    """The `sampler` argument of Evaluation.ppl.PPL_Distances for case c."""
    def sample(batch_index, batch_size, latent_dim, device):
        assert (batch_size, latent_dim) == (c['batch'], c['latent_dim'])
        z, t = inputs(c, batch_index)
        return z.to(device=device, dtype=dtype), t.to(device=device, dtype=dtype)
    return sample


def standin_distance(x, y):
    return ((x - y) ** 2).mean([1, 2, 3])


class ToyGenerator(nn.Module):
    """A two-layer mapping network `style` and a linear map to [N, 3, 8, 8] behind a tanh; takes the Generator's call."""

    def __init__(self, latent_dim=16):
        super().__init__()
        self.style = nn.Sequential(nn.Linear(latent_dim, latent_dim), nn.LeakyReLU(0.2), nn.Linear(latent_dim, latent_dim))
        self.to_image = nn.Linear(latent_dim, 3 * 8 * 8)
        sd = {}
        for k, v in self.state_dict().items():
            scale = 0.1 if v.ndim == 1 else (1.0 / v.shape[1]) ** 0.5
            sd[k] = synth.tensor('ppl/toy_generator/' + k, v.shape, scale=scale)
        self.load_state_dict(sd)
        self.eval().requires_grad_(False)

    def forward(self, noise_z=None, latent_styles=None, input_is_latent=True, noise=None, **kw):
        assert noise_z is None and input_is_latent and noise is None and len(latent_styles) == 1
        return torch.tanh(self.to_image(latent_styles[0])).view(-1, 3, 8, 8)


def percept_state_dict(ref_sd):
    """Weights for lpips.PerceptualLoss, entry by entry: the ScalingLayer buffers stay; 3x3 convs N(0, 2 / fan_in), biases
    N(0, 0.1^2); the 1x1 layers |N(0, 1)| (the reference keeps them non-negative)."""
    out = {}
    for key, ref in ref_sd.items():
        if 'scaling_layer' in key:
            out[key] = ref.clone()
        elif '.model.' in key:
            out[key] = synth.tensor('ppl/lpips/' + key, ref.shape, dtype=ref.dtype).abs()
        elif ref.ndim == 4:
            fan_in = ref.shape[1] * ref.shape[2] * ref.shape[3]
            out[key] = synth.tensor('ppl/lpips/' + key, ref.shape, scale=(2.0 / fan_in) ** 0.5, dtype=ref.dtype)
        else:
            out[key] = synth.tensor('ppl/lpips/' + key, ref.shape, scale=0.1, dtype=ref.dtype)
    return out
