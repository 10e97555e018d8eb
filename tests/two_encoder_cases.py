"""Cases and builders of the 2-encoder scheme, shared by tools/make_golden_two_encoder.py (reference side, CPU) and the
tests: (tensor encoder, modulation encoder, Generator) per mode, their synthetic state dicts and checkpoints, inputs.
Fixture: tests/golden/two_encoder.npz (outputs only: strided samples, stats, float64 samples, gradient samples).

The builders take the modules to build from (`resnet_encoder`, `psp_encoders`, `stylegan2`) as arguments: the tool passes
the reference's, the tests this package's; constructor arguments and state-dict names are the same on both sides."""
import math
import types

import synth

CONCAT_MODES = ('Concatenation', 'Tensor Transform')
# synth's rule gives ten_fc.weight [512, 8192] unit scale: the 512-vector of 'Tensor Transform' then has a standard
# deviation near sqrt(8192) * |activation| and the image a magnitude of several hundred, against 5-13 in the other
# modes.  Both sides multiply ten_fc.weight and ten_fc.bias by this (a power of two: exact), after synth has filled them.
TEN_FC_SCALE = 2.0 ** -6

# B = 2, 256^2 inputs, Generator(256): the four modes of Forward_Inference
FORWARD_CASES = [
    dict(name='plain_w_render', size=256, b=2, mod_space='W', mod_encode='Render Image', co_mod=None, sliced_layer=None,
         use_tanh=False, stride=16),
    dict(name='plain_wplus_photo', size=256, b=2, mod_space='W+', mod_encode='Photo Image', co_mod=None,
         sliced_layer=None, use_tanh=False, stride=16),
    dict(name='mult_sliced', size=256, b=2, mod_space='W+', mod_encode='Render Image', co_mod='Multiplication',
         sliced_layer=[1, 2, 5], use_tanh=False, stride=16),
    dict(name='concat', size=256, b=2, mod_space='W+', mod_encode='Render Image', co_mod='Concatenation',
         sliced_layer=None, use_tanh=False, stride=16),
    dict(name='tensor_transform_tanh', size=256, b=2, mod_space='W+', mod_encode='Render Image',
         co_mod='Tensor Transform', sliced_layer=None, use_tanh=True, stride=16),
]

# ONE photo, 3 render frames (chunk 2 in the tests: a ragged last chunk); the reference runs frame by frame with the photo
REANIMATE_CASES = [
    dict(name='re_mult', size=256, frames=3, mod_space='W+', mod_encode='Render Image', co_mod='Multiplication',
         sliced_layer=list(range(4, 14)), use_tanh=False, stride=16),
    dict(name='re_concat', size=256, frames=3, mod_space='W+', mod_encode='Render Image', co_mod='Concatenation',
         sliced_layer=None, use_tanh=False, stride=16),
    dict(name='re_tensor_transform', size=256, frames=3, mod_space='W+', mod_encode='Render Image',
         co_mod='Tensor Transform', sliced_layer=None, use_tanh=True, stride=16),
    dict(name='re_plain_render', size=256, frames=3, mod_space='W', mod_encode='Render Image', co_mod=None,
         sliced_layer=None, use_tanh=False, stride=16),
]

# forward + backward: L1 loss to a synthetic target, every parameter gradient of the three modules
GRAD_CASE = dict(name='two_enc_grad', size=64, b=2, mod_space='W+', mod_encode='Render Image', co_mod='Tensor Transform',
                 sliced_layer=None, use_tanh=False, stride=4)


def style_dim(c):
    return 1024 if c['co_mod'] in CONCAT_MODES else 512


def n_styles(size):
    return int(math.log2(size)) * 2 - 2


def uses_psp(c):
    return c['co_mod'] is not None or c['mod_space'] == 'W+'


def modules(c, resnet_encoder, psp_encoders, stylegan2, depth=18):
    """(tensor encoder, modulation encoder, Generator) of a case as freshly constructed modules."""
    if c['co_mod'] is None:
        e_tsr = resnet_encoder.resnet18(tensor_encoding=True)
    elif c['co_mod'] == 'Tensor Transform':
        e_tsr = resnet_encoder.resnet18(tensor_encoding=True, tensor_transform=True)
    else:
        e_tsr = resnet_encoder.resnet18(tensor_encoding=False)
    if uses_psp(c):
        opts = types.SimpleNamespace(input_nc=3, n_styles=n_styles(c['size']))
        e_w = psp_encoders.GradualStyleEncoder(depth, 'ir_se', opts)
    else:
        e_w = resnet_encoder.resnet18(tensor_encoding=False)
    return e_tsr, e_w, stylegan2.Generator(c['size'], style_dim(c), 8)


def state_dicts(c, e_tsr, e_w, g):
    """{'e_tsr', 'e_W', 'g_ema'}: synth's state dicts of the three modules, with the seeds of the other fixtures and
    ten_fc scaled by TEN_FC_SCALE."""
    sd_t = synth.state_dict('resnet', e_tsr.state_dict(), seed=5)
    for k in ('ten_fc.weight', 'ten_fc.bias'):
        if k in sd_t:
            sd_t[k] = sd_t[k] * TEN_FC_SCALE
    sd_w = (synth.state_dict('psp', e_w.state_dict(), seed=7) if uses_psp(c)
            else synth.state_dict('resnet', e_w.state_dict(), seed=6))
    return dict(e_tsr=sd_t, e_W=sd_w, g_ema=synth.state_dict('generator', g.state_dict(), seed=4))


def build(c, resnet_encoder, psp_encoders, stylegan2):
    """The three modules of a case with their synthetic weights, in eval mode, on the CPU in float32."""
    mods = modules(c, resnet_encoder, psp_encoders, stylegan2)
    sds = state_dicts(c, *mods)
    for m, k in zip(mods, ('e_tsr', 'e_W', 'g_ema')):
        m.load_state_dict(sds[k])
        m.eval()
    return mods


def checkpoint(c, resnet_encoder, psp_encoders, stylegan2, depth=18, mode_keys=True):
    """A checkpoint dict as the reference's train.py writes it (the keys an inference model is built from)."""
    ckpt = state_dicts(c, *modules(c, resnet_encoder, psp_encoders, stylegan2, depth))
    if mode_keys:
        ckpt.update(mod_space=c['mod_space'], mod_encode=c['mod_encode'],
                    co_mod=True if c['co_mod'] == 'Multiplication' else c['co_mod'])
    return ckpt


def inputs(c):
    """(photo, render) [b,3,256,256] of a forward or gradient case, U(-1,1)."""
    p = synth.tensor(c['name'] + '/photo', (c['b'], 3, 256, 256), dist='uniform')
    r = synth.tensor(c['name'] + '/render', (c['b'], 3, 256, 256), dist='uniform')
    return p, r


def reanimate_inputs(c):
    """(photo [1,3,256,256], renders [frames,3,256,256]) of a re-animation case, U(-1,1)."""
    p = synth.tensor(c['name'] + '/photo', (1, 3, 256, 256), dist='uniform')
    r = synth.tensor(c['name'] + '/render', (c['frames'], 3, 256, 256), dist='uniform')
    return p, r


def target(c):
    return synth.tensor(c['name'] + '/target', (c['b'], 3, c['size'], c['size']), dist='uniform')
