"""The library handle and the networks the tests build, with tests/synth.py's weights (not a conftest: plain helpers,
imported by name).  Every call returns fresh objects: a cache here would keep GPU memory alive across test modules, and
op/placement.py's ballast guard reads free memory.  Caching belongs to the test files' own fixtures and dictionaries."""
import types

import torch

import ppl_cases as pc
import synth
from gpumem import dev


def lib():
    from op import _native
    return _native.lib()


def load(module, kind, seed, eval=True):
    """`module` with synth's state dict of `kind` and `seed`, on the device; in eval mode unless eval=False (which
    leaves the module's mode as it is)."""
    module.load_state_dict(synth.state_dict(kind, module.state_dict(), seed=seed))
    module = module.to(dev())
    return module.eval() if eval else module


def encoders(n_styles):
    """(E_Tsr, E_W, E_W_Plus) with the seeds of the golden fixtures."""
    import resnet_encoder
    from psp_encoder_model.encoders import psp_encoders
    e_tsr = load(resnet_encoder.resnet18(tensor_encoding=True, tensor_transform=False), 'resnet', 5)
    e_w = load(resnet_encoder.resnet18(tensor_encoding=False, tensor_transform=False), 'resnet', 6)
    e_wp = load(psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=n_styles)),
                'psp', 7)
    return e_tsr, e_w, e_wp


def percept(device=None):
    """lpips' VGG net-lin model with the stand-in weights of tests/ppl_cases.py: on the CPU, or on `device` in
    channels_last."""
    import lpips
    p = lpips.PerceptualLoss(model='net-lin', net='vgg')
    p.load_state_dict(pc.percept_state_dict(p.state_dict()))
    return p if device is None else p.to(device).to(memory_format=torch.channels_last)


def scaling():
    import lpips
    return lpips.ScalingLayer().to(dev())


class PinNoise(torch.nn.Module):
    """Forward_Inference_3_Encoder never passes noise; the fixtures pinned randomize_noise=False.
    `.module` is what the reference reads n_latent from (Util/network_util.py:317-318)."""

    def __init__(self, g, call=None):
        super().__init__()
        self.module = g
        self._call = [call if call is not None else g]      # in a list: not a registered submodule twice

    def forward(self, **kw):
        return self._call[0](randomize_noise=False, **kw)
