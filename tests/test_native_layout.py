"""The layout of the package op/_native: every name the one-file module offered is still `_native.<name>`, the package
state (observer, the two ambient switches) has one owner that every family module reads at call time, and the switches
nest and restore."""
import pytest
import torch

import launches
import synth

# dir(op._native) of the last one-file version: every name without a leading underscore, the imported modules left out;
# plus the wrappers added since (modconv_wgrad_select).
PUBLIC_NAMES = (
    'BANK_GATHER_BANKS', 'BANK_GATHER_GROUPS', 'BF16', 'BLUR_PATHS', 'EMA_CHUNK', 'F16', 'F32', 'F64', 'FMGAN_EINVAL',
    'FMGAN_EUNSUPPORTED', 'FMGAN_OK', 'HEATMAP_SIZE', 'INCEPTION_SIZE', 'LIB_PATH', 'LOSS_ROW_COLUMNS', 'LPIPS_SIZE',
    'activation_io', 'aligned_rows_buffer', 'aligned_rows_shape', 'amp_bwd', 'amp_fwd', 'amp_fwd_io', 'bank_gather',
    'blur_noise_bias_act', 'blur_noise_bias_act_serves', 'bn_prelu', 'check', 'conv3x3s2_bf16x3',
    'conv3x3s2_bf16x3_supported', 'conv_weight_to_bf16x3', 'current_activation_io', 'current_modconv_precision',
    'demod_bank', 'detector_input', 'dtype16_code', 'dtype_code', 'ema', 'ema_blocks', 'equal_linear', 'f64p',
    'face_crop_bwd', 'face_crop_fwd', 'face_crop_serves', 'face_input', 'face_input_pool', 'face_region_loss',
    'face_region_loss_backward', 'fid_stats_finish', 'fid_stats_serves', 'fid_stats_update', 'fp', 'fused_bias_act',
    'fused_bias_act16', 'fused_bias_act16_backward', 'fused_bias_act_backward', 'heatmap_distance_bwd',
    'heatmap_distance_fwd', 'heatmap_distance_serves', 'images_to_tensor', 'inception_input', 'io16', 'ir_tail',
    'landmark_decode', 'launching', 'lbfgs_coeffs', 'lbfgs_direction', 'lbfgs_gather', 'lbfgs_pair', 'lbfgs_segments',
    'lbfgs_update', 'lib', 'loss_row', 'lpips_distance', 'lpips_distance_backward', 'lpips_pair_input', 'modconv2d',
    'modconv2d_rgb', 'modconv2d_rgb_fusable', 'modconv2d_select', 'modconv2d_tiles', 'modconv2d_winograd',
    'modconv_demod', 'modconv_precision', 'modconv_weight_prep', 'modconv_weight_to_bf16', 'modconv_weight_to_bf16x3',
    'modconv_wgrad', 'modconv_wgrad_select', 'modconv_wsq', 'nhwc_dense', 'noise_bias_act', 'on_device', 'prelu_backward', 'projection_loss_bwd',
    'projection_loss_fwd', 'ptr', 'render_mask', 'require_f32_gpu', 'require_gpu', 'resize_images', 'resize_output_size',
    'resize_plan', 'se_gate', 'se_pool', 'served', 'set_observer', 'style_bank', 'tensor_to_images', 'tiles_to_canvas',
    'torgb', 'torgb_backward', 'upfirdn2d', 'upfirdn2d16', 'upfirdn2d_out_size', 'upfirdn2d_strided', 'wino_input',
    'wino_output', 'wino_weight')
# the ones that are values, with the values they had (LIB_PATH: where the library is, checked apart)
CONSTANTS = dict(BANK_GATHER_BANKS=4, BANK_GATHER_GROUPS=8, BF16=3, BLUR_PATHS={}, EMA_CHUNK=4096, F16=2, F32=0, F64=1,
                 FMGAN_EINVAL=-1, FMGAN_EUNSUPPORTED=-2, FMGAN_OK=0, HEATMAP_SIZE=64, INCEPTION_SIZE=299,
                 LOSS_ROW_COLUMNS=16, LPIPS_SIZE=256)
FAMILIES = ('activation', 'conv', 'encoder', 'loss', 'evaluation', 'image', 'optim')


def test_every_public_name_is_a_package_attribute():
    import os
    from op import _native
    assert len(set(PUBLIC_NAMES)) == len(PUBLIC_NAMES) == 118
    missing = [n for n in PUBLIC_NAMES if not hasattr(_native, n)]
    assert not missing, missing
    for name in PUBLIC_NAMES:
        value = getattr(_native, name)
        if name in CONSTANTS:
            assert value == CONSTANTS[name] and type(value) is type(CONSTANTS[name]), name
        elif name == 'LIB_PATH':
            op_dir = os.path.dirname(os.path.dirname(os.path.abspath(_native.__file__)))
            assert value == (os.environ.get('FMGAN_LIB') or os.path.join(os.path.dirname(op_dir), 'csrc', 'libfmgan_hip.so'))
        else:
            assert callable(value), name
    # a re-exported object is its owner's: what bench.py reads as _native.BLUR_PATHS is the dict the wrapper fills
    assert _native.BLUR_PATHS is _native.activation.BLUR_PATHS
    assert _native.lib() is _native.core._lib


def test_observer_has_one_owner():
    """set_observer rebinds core._observer; a family module that copied the name at import would keep the old one."""
    from op import _native
    core = _native.core
    for family in FAMILIES:
        assert '_observer' not in vars(getattr(_native, family)), family
    rec = launches.Recorder()
    _native.set_observer(rec)
    try:
        assert core._observer is rec
    finally:
        _native.set_observer(None)
    assert isinstance(core._observer, core._NullObserver)


@pytest.mark.gpu
def test_installed_observer_sees_another_modules_bracket():
    from op import _native
    core = _native.core
    d = torch.device('cuda', 0)
    x = synth.tensor('layout/nba/x', (1, 4, 8, 8)).to(d)
    bias = synth.tensor('layout/nba/b', (4,)).to(d)
    rec = launches.Recorder()
    _native.set_observer(rec)
    try:
        _native.noise_bias_act(x, None, None, bias, 0.2, 2 ** 0.5)               # op/_native/activation.py
    finally:
        _native.set_observer(None)
    assert rec.seen == [('noise_bias_act', (256, 4))]
    assert isinstance(core._observer, core._NullObserver)
    _native.noise_bias_act(x, None, None, bias, 0.2, 2 ** 0.5)
    assert len(rec.seen) == 1                                                    # the removed observer hears no more


@pytest.mark.parametrize('switch,current,owner,var,values,text', [
    ('modconv_precision', 'current_modconv_precision', 'conv', '_mc_precision', ('f32', 'bf16', 'bf16x3'),
     "precision must be 'f32', 'bf16' or 'bf16x3'"),
    ('activation_io', 'current_activation_io', 'activation', '_act_io', ('fp32', '16'), "mode must be 'fp32' or '16'"),
], ids=['modconv_precision', 'activation_io'])
def test_ambient_switches_nest_and_restore(switch, current, owner, var, values, text):
    from op import _native
    switch, current, owner = getattr(_native, switch), getattr(_native, current), getattr(_native, owner)
    default, other = values[0], values[-1]
    assert current() == default == getattr(owner, var)
    with switch(other) as entered:
        assert isinstance(entered, switch)
        assert current() == other == getattr(owner, var)
        with switch(default):
            assert current() == default
            with switch(other):
                assert current() == other
            assert current() == default
        assert current() == other
        with pytest.raises(KeyError):
            with switch(default):
                assert current() == default
                raise KeyError('body')
        assert current() == other                     # the inner switch put `other` back although its body raised
    assert current() == default == getattr(owner, var)
    for value in values:
        with switch(value):
            assert current() == value
    for bad in ('fp16', None, 16, ''):
        with pytest.raises(ValueError) as e:
            switch(bad)
        assert str(e.value) == text
    assert current() == default
