"""Image-projection cases shared by tools/make_golden_projection.py (reference side) and the tests.  Fixture:
tests/golden/projection.npz, outputs only, each from the reference's own code on the CPU in fp32 and in float64.

Criterion cases (`CRITERION_CASES`): one ImageReconstructionLoss per case and a sequence of calls on it.  Per call i:
    <name>/<i>/loss, /loss64        the value of the fp32 and of the float64 run
    <name>/<i>/grad64               the float64 gradient with respect to `output`, sampled [:, :, ::s, ::s] (s = `stride`)
    <name>/<i>/grad_max64           max |grad64| over the whole tensor
    <name>/<i>/grad_err             max |grad32 - grad64| over the whole tensor: the reference's own fp32 error
    <name>/<i>/use_lpips            whether LPIPS was on in that call
Inputs come from tests/synth.py on both sides (`criterion_inputs`): the target is U(-1, 1); a seventh of its values
is stretched by 1.6 (a third of those beyond +-1) and some are exactly +-1; the output of call i is target +
amplitude_i * N(0, 1), again exactly +-1 at those places (the clamp's two branches and its boundary).  The amplitudes of
the `mix` case take the mse term across the 0.01 threshold between calls: 0.5 (mse 0.25: off), 0.05 (mse 0.0025: LPIPS
joins), 0.5 again (stays on).  The perceptual module is the project's lpips.PerceptualLoss on both sides with the weights
of ppl_cases.percept_state_dict.  With a mask only 'mse' is defined (the reference hands the mask to the perceptual
module as `normalize`, which fails).

Trajectories (`TRAJECTORIES`): the reference's optimize with Adam(lr=0.01), set up as Image_Projector does (avg_W from the
mapping network over fixed samples, repeated per image; noise maps; latent and noises optimised), against
ImageReconstructionLoss('mse+lpips').  `toy` uses ToyProjGenerator, which also runs on the CPU; the others a narrow
Generator (channel_multiplier 1, a two-layer mapping network) in W or W+.  Per trajectory:
    <name>/lr                       the learning rate of every step (iterations + 1 of them)
    <name>/loss, /loss64            the loss of every step
    <name>/dW64, /dnoise<i>64       final - initial of the float64 run (maps wider than 32 sampled [::s, ::s], s = w // 32)
    <name>/dW_err, /dnoise_err      relative L2 error of the fp32 run's displacement against the float64 run's (W; per map)
The tool asserts that every figure of dW_err, dnoise_err and the relative loss errors stays within 1e-2; if one does not,
the iterations here are reduced.
"""
import torch
from torch import nn

import synth

CRITERION_CASES = [
    dict(name='c64_mse_mask', size=64, batch=2, loss='mse', mask=True, amplitudes=(0.3,), stride=5),
    dict(name='c64_lpips', size=64, batch=1, loss='mse+lpips', mask=False, amplitudes=(0.3,), stride=5),
    dict(name='c256_mse', size=256, batch=2, loss='mse', mask=False, amplitudes=(0.3,), stride=11),
    dict(name='c256_mse_mask', size=256, batch=1, loss='mse', mask=True, amplitudes=(0.3,), stride=11),
    dict(name='c256_lpips', size=256, batch=2, loss='mse+lpips', mask=False, amplitudes=(0.3,), stride=11),
    dict(name='c256_mix', size=256, batch=1, loss='mse+lpips+mix', mask=False, amplitudes=(0.5, 0.05, 0.5), stride=11),
    dict(name='c512_mse_mask', size=512, batch=1, loss='mse', mask=True, amplitudes=(0.3,), stride=23),
    dict(name='c512_lpips', size=512, batch=1, loss='mse+lpips', mask=False, amplitudes=(0.3,), stride=23),
]
CRITERION_BY_NAME = {c['name']: c for c in CRITERION_CASES}

TRAJECTORIES = [
    dict(name='toy', kind='toy', size=16, batch=1, per_layer=False, iterations=3, n_avg=16),
    dict(name='g64_w', kind='generator', size=64, batch=2, per_layer=False, iterations=6, n_avg=16),
    dict(name='g64_wplus', kind='generator', size=64, batch=2, per_layer=True, iterations=6, n_avg=16),
    dict(name='g256_w', kind='generator', size=256, batch=1, per_layer=False, iterations=4, n_avg=16),
]
TRAJECTORY_BY_NAME = {c['name']: c for c in TRAJECTORIES}
LATENT_DIM = 512
TOY_DIM = 16
LR = 0.01


def criterion_inputs(c, call, dtype=torch.float32):
    """(output, target, mask or None) of call `call` of criterion case c, on the CPU."""
    shape = (c['batch'], 3, c['size'], c['size'])
    target = synth.tensor(f"projection/{c['name']}/target", shape, dist='uniform')
    flat = target.view(-1)
    flat[0::7] = flat[0::7] * 1.6            # a third of these beyond +-1: the clamp stops the LPIPS gradient there
    flat[1::101] = 1.0
    flat[2::103] = -1.0
    output = target + c['amplitudes'][call] * synth.tensor(f"projection/{c['name']}/noise/{call}", shape)
    flat = output.view(-1)
    flat[1::101] = 1.0                       # exactly on the bounds: the gradient passes
    flat[2::103] = -1.0
    mask = None
    if c['mask']:
        m = (synth.tensor(f"projection/{c['name']}/mask", shape[2:], dist='uniform') + 1) / 2
        mask = torch.where(m < 0.25, torch.zeros_like(m), m).to(dtype)
    return output.to(dtype), target.to(dtype), mask


def image_pair(index, size=512):
    """Two images on the 0..255 scale (float64 numpy, [1, 3, size, size]) for psnr, and as tensors in [-1, 1] for
    Downsample_Image_256."""
    a = synth.tensor(f'projection/helpers/a/{index}', (1, 3, size, size), dist='uniform')
    b = (a + 0.1 * synth.tensor(f'projection/helpers/b/{index}', (1, 3, size, size))).clamp(-1, 1)
    return a, b


def down_input(index):
    """Input of Downsample_Image_256: a 512^2 image (one halving) and a 1024^2 one (two)."""
    a, b = image_pair(index)
    return a if index == 0 else b.repeat(1, 1, 2, 2)


def to_255(t):
    return ((t.double() + 1) * 127.5).numpy()


class ToyProjGenerator(nn.Module):
    """What Image_Projector needs of a Generator, small enough for the CPU: a two-layer mapping network `style`,
    make_noise, num_layers, style_dim, and a forward that takes the Generator's projection call.  The image is
    tanh(linear(latent)) plus the noise maps (nearest-upsampled to the image size) times fixed weights."""
    size = 16

    def __init__(self, style_dim=TOY_DIM):
        super().__init__()
        self.style_dim, self.num_layers = style_dim, 2
        self.style = nn.Sequential(nn.Linear(style_dim, style_dim), nn.LeakyReLU(0.2), nn.Linear(style_dim, style_dim))
        self.to_image = nn.Linear(style_dim, 3 * self.size * self.size)
        self.noise_weight = nn.Parameter(torch.zeros(2, 3))
        sd = {}
        for k, v in self.state_dict().items():
            scale = 0.1 if v.ndim == 1 else (1.0 / v.shape[1]) ** 0.5
            sd[k] = synth.tensor('projection/toy_generator/' + k, v.shape, scale=scale)
        self.load_state_dict(sd)
        self.eval().requires_grad_(False)

    def make_noise(self):
        p = self.to_image.weight
        return [torch.randn(1, 1, 8, 8, device=p.device, dtype=p.dtype),
                torch.randn(1, 1, 16, 16, device=p.device, dtype=p.dtype)]

    def forward(self, noise_z=None, latent_styles=None, input_is_latent=True, noise=None, **kw):
        assert noise_z is None and input_is_latent and len(latent_styles) == 1 and len(noise) == 2
        w = latent_styles[0]
        w = w.mean(1) if w.ndim == 3 else w
        image = torch.tanh(self.to_image(w)).view(-1, 3, self.size, self.size)
        for i, nz in enumerate(noise):
            up = nn.functional.interpolate(nz, size=self.size, mode='nearest')
            image = image + self.noise_weight[i].view(1, 3, 1, 1) * up
        return image


def trajectory_start(c, generator, dtype=torch.float32, device='cpu'):
    """(avg_W, noises, target) as Image_Projector sets them up, from fixed samples: avg_W [B, D] or [B, n_latent, D] is the
    mean of generator.style over n_avg synth samples, repeated; the noise maps have the shapes of generator.make_noise();
    the target is U(-0.9, 0.9), smooth enough to sit inside the clamp."""
    z = synth.tensor(f"projection/{c['name']}/z", (c['n_avg'], generator.style_dim)).to(device=device, dtype=dtype)
    with torch.no_grad():
        avg = generator.style(z).mean(0)
        shapes = [tuple(n.shape) for n in generator.make_noise()]
    if c['per_layer']:
        avg = avg.repeat((generator.num_layers + 1, 1)).unsqueeze(0)
    else:
        avg = avg.reshape(1, -1)
    avg_w = torch.repeat_interleave(avg, c['batch'], dim=0).clone()
    noises = [synth.tensor(f"projection/{c['name']}/noise{i}", s).to(device=device, dtype=dtype)
              for i, s in enumerate(shapes)]
    target = 0.9 * synth.tensor(f"projection/{c['name']}/target", (c['batch'], 3, c['size'], c['size']), dist='uniform')
    return avg_w, noises, target.to(device=device, dtype=dtype)


def noise_sample(d):
    """The stored part of a displacement: all of W and of a noise map [1, 1, h, w] up to 32 wide, else every (w // 32)-th
    row and column."""
    s = max(d.shape[-1] // 32, 1) if d.ndim == 4 else 1
    return d[..., ::s, ::s]
