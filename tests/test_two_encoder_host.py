"""CPU tests of the 2-encoder scheme's host side: Model_Building_Func_2_Encoder on synthetic checkpoints, the argument
checks of Forward_Inference and of Table.run_concat (before any launch), the concatenating entry point's refusals, and
that the product imports nothing from oracle/."""
import ast
import ctypes
import os

import pytest
import torch

import two_encoder_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c['name']: c for c in tc.FORWARD_CASES}


def _ckpt(name, **kw):
    import resnet_encoder
    import stylegan2
    from psp_encoder_model.encoders import psp_encoders
    return tc.checkpoint(BY_NAME[name], resnet_encoder, psp_encoders, stylegan2, **kw)


def _bare_eval(*mods):
    for m in mods:
        assert isinstance(m, torch.nn.Module) and not hasattr(m, 'module') and not m.training
        assert all(p.device.type == 'cpu' for p in m.parameters())


def test_model_building_defaults_without_mode_keys():
    import resnet_encoder
    import stylegan2
    from Util.analysis_util import Model_Building_Func_2_Encoder
    ckpt = _ckpt('plain_w_render', mode_keys=False)
    assert not {'mod_space', 'mod_encode', 'co_mod'} & set(ckpt)
    g_ema, E_Tsr, E_W, mod_encode, co_mod = Model_Building_Func_2_Encoder(ckpt, 'cpu')
    assert (mod_encode, co_mod) == ('Render Image', None)
    _bare_eval(g_ema, E_Tsr, E_W)
    assert isinstance(g_ema, stylegan2.Generator) and (g_ema.size, g_ema.style_dim) == (256, 512)
    assert isinstance(E_Tsr, resnet_encoder.ResNet) and E_Tsr.tensor_encoding and not E_Tsr.tensor_transform
    assert isinstance(E_W, resnet_encoder.ResNet) and not E_W.tensor_encoding
    for m, k in ((g_ema, 'g_ema'), (E_Tsr, 'e_tsr'), (E_W, 'e_W')):                # the checkpoint's values were loaded
        sd = m.state_dict()
        assert all(torch.equal(sd[n], v) for n, v in ckpt[k].items())
    # gpu_device_ids is accepted and ignored
    assert Model_Building_Func_2_Encoder(ckpt, 'cpu', [0])[3:] == ('Render Image', None)


def test_model_building_plain_wplus_photo():
    from psp_encoder_model.encoders import psp_encoders
    from Util.analysis_util import Model_Building_Func_2_Encoder
    g_ema, E_Tsr, E_W, mod_encode, co_mod = Model_Building_Func_2_Encoder(_ckpt('plain_wplus_photo'), 'cpu')
    assert (mod_encode, co_mod) == ('Photo Image', None)
    assert E_Tsr.tensor_encoding and isinstance(E_W, psp_encoders.GradualStyleEncoder)
    assert (E_W.num_layers, E_W.style_count, g_ema.style_dim) == (18, 14, 512)


def test_model_building_co_mod_true_is_multiplication():
    from psp_encoder_model.encoders import psp_encoders
    from Util.analysis_util import Model_Building_Func_2_Encoder
    ckpt = _ckpt('mult_sliced')
    assert ckpt['co_mod'] is True and len(ckpt['e_W']) == 325
    g_ema, E_Tsr, E_W, mod_encode, co_mod = Model_Building_Func_2_Encoder(ckpt, 'cpu')
    assert (mod_encode, co_mod) == ('Render Image', 'Multiplication')
    _bare_eval(g_ema, E_Tsr, E_W)
    assert g_ema.style_dim == 512 and not E_Tsr.tensor_encoding and not hasattr(E_Tsr, 'ten_fc')
    assert isinstance(E_W, psp_encoders.GradualStyleEncoder) and (E_W.num_layers, E_W.style_count) == (18, 14)


@pytest.mark.parametrize('name', ['concat', 'tensor_transform_tanh'])
def test_model_building_concatenating_modes(name):
    from Util.analysis_util import Model_Building_Func_2_Encoder
    c = BY_NAME[name]
    g_ema, E_Tsr, E_W, mod_encode, co_mod = Model_Building_Func_2_Encoder(_ckpt(name), 'cpu')
    assert co_mod == c['co_mod'] and mod_encode == c['mod_encode']
    _bare_eval(g_ema, E_Tsr, E_W)
    assert g_ema.style_dim == 1024 and tuple(g_ema.conv1.conv.modulation.weight.shape) == (512, 1024)
    transform = c['co_mod'] == 'Tensor Transform'
    assert hasattr(E_Tsr, 'ten_fc') == transform == E_Tsr.tensor_transform == E_Tsr.tensor_encoding
    assert E_W.num_layers == 18


def test_model_building_reads_the_psp_depth_off_the_body():
    from Util.analysis_util import Model_Building_Func_2_Encoder, _psp_depth
    ckpt = _ckpt('mult_sliced', depth=50)
    assert len(ckpt['e_W']) == 565 and _psp_depth(ckpt['e_W']) == 50
    E_W = Model_Building_Func_2_Encoder(ckpt, 'cpu')[2]
    assert E_W.num_layers == 50 and len(E_W.body) == 24 and not E_W.training
    # another number of style heads changes the key count, not the depth
    fewer = {k: v for k, v in ckpt['e_W'].items() if not k.startswith('styles.13.')}
    assert len(fewer) not in (325, 565) and _psp_depth(fewer) == 50
    # an unrecognisable body: ValueError naming the count, not the reference's unbound name
    broken = dict(ckpt, e_W={k: v for k, v in ckpt['e_W'].items() if not k.startswith('body.23.')})
    with pytest.raises(ValueError) as e:
        Model_Building_Func_2_Encoder(broken, 'cpu')
    assert str(len(broken['e_W'])) in str(e.value) and '23' in str(e.value)
    with pytest.raises(ValueError):
        Model_Building_Func_2_Encoder(dict(ckpt, co_mod='Addition'), 'cpu')


def test_forward_inference_validates_its_modes_before_any_encoder_runs():
    from Util.network_util import (CO_MODULATION_MODE, Encode_Photo_2_Encoder, Forward_Inference,
                                   Forward_Inference_Reanimate_2_Encoder, PhotoCode2, Reanimate_From_Codes_2_Encoder)
    assert CO_MODULATION_MODE == ['Multiplication', 'Concatenation', 'Tensor Transform']

    def never(x):
        raise AssertionError('an encoder ran')

    x = torch.zeros(1, 3, 256, 256)
    for kw in (dict(mod_encode='Both'), dict(co_modulation='Addition'), dict(co_modulation=True),
               dict(mod_encode=None, co_modulation='Concatenation')):
        with pytest.raises(ValueError):
            Forward_Inference(x, x, never, never, never, **kw)
        with pytest.raises(ValueError):
            Encode_Photo_2_Encoder(x, never, never, **kw)
        with pytest.raises(ValueError):
            Forward_Inference_Reanimate_2_Encoder(PhotoCode2(None, None), x, never, never, never, **kw)
        with pytest.raises(ValueError):
            Reanimate_From_Codes_2_Encoder(PhotoCode2(None, None), x, never, **kw)
    # re-animation has no CPU path
    with pytest.raises(RuntimeError):
        Encode_Photo_2_Encoder(x, never, never, 'Render Image', 'Concatenation')
    with pytest.raises(RuntimeError):
        Forward_Inference_Reanimate_2_Encoder(PhotoCode2(None, None), x, never, never, never)


def test_reanimate_frames_2_encoder_wants_three_modules():
    from Evaluation.visual_eval import Reanimate_Frames_2_Encoder
    x = torch.zeros(1, 3, 256, 256)
    with pytest.raises(ValueError):
        Reanimate_Frames_2_Encoder(x, x, (None,) * 4)
    with pytest.raises(ValueError):
        Reanimate_Frames_2_Encoder(x, x, (None,) * 3, chunk=0)


def _table(style_dim=96, n_styles=7, cols=(0, 1, 6)):
    """A Table as its constructor leaves it, without device memory: run_concat's checks come before any launch."""
    from op.style_bank import Table
    t = Table.__new__(Table)
    t.n, t.n_styles, t.style_dim, t.cols = len(cols), n_styles, style_dim, list(cols)
    t.style_floats, t.demod_floats, t.dev = 8, 4, torch.zeros(1, dtype=torch.uint8)
    return t


def test_table_run_concat_checks_dimensions_before_any_launch(monkeypatch):
    from op import _native

    def never(*a, **kw):
        raise AssertionError('a launch was reached')
    monkeypatch.setattr(_native, 'style_bank_concat', never)
    monkeypatch.setattr(_native, 'demod_bank', never)
    T = 3
    v, wp = torch.zeros(T, 32), torch.zeros(1, 7, 64)
    styles, demod = torch.zeros(T * 8), torch.zeros(T * 4)
    bad = [(_table(), (v[:, :-1], wp, styles, demod)),                      # Dv + Dw != style_dim
           (_table(), (v, wp[:, :, :-1], styles, demod)),
           (_table(), (v, wp[:, :6], styles, demod)),                       # W+ columns != the table's
           (_table(), (v, wp.expand(2, -1, -1), styles, demod)),            # P not in {1, T}
           (_table(), (v, wp[0], styles, demod)),                           # W+ not [P, n, Dw]
           (_table(), (v, wp, styles[:-1], demod)),                         # short buffers
           (_table(), (v, wp, styles, demod[:-1])),
           (_table(cols=(0, 7)), (v, wp, styles, demod))]                   # a column W+ does not have
    for table, args in bad:
        with pytest.raises(RuntimeError):
            table.run_concat(*args)
    with pytest.raises(AssertionError):                                     # the accepted shapes do reach the launch
        _table().run_concat(v, wp, styles, demod)


def test_concat_entry_point_refuses_bad_arguments_without_gpu():
    """EINVAL before any HIP call; batch == 0 is a no-op (as tests/test_style_bank_host.py for the multiplicative one)."""
    from op import _native
    L = _native.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(table=p, n=1, v=p, wplus=p, wb=1, batch=2, dv=3, dw=5, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.fmgan_style_bank_concat_f32(a['table'], a['n'], a['v'], a['wplus'], a['wb'], a['batch'], a['dv'], a['dw'],
                                             a['out'], None)
    for kw in (dict(table=None), dict(v=None), dict(wplus=None), dict(out=None), dict(n=0), dict(n=65536), dict(wb=3),
               dict(wb=0), dict(dv=0), dict(dw=0), dict(dv=-1), dict(batch=-1)):
        assert call(**kw) == _native.FMGAN_EINVAL, kw
    assert call(batch=0) == _native.FMGAN_OK
    assert call(batch=0, table=None, v=None, wplus=None, out=None) == _native.FMGAN_OK


def test_concat_column_is_the_materialised_latent_column():
    from op.style_bank import concat_column
    v = torch.arange(6.).reshape(3, 2)
    for wp in (torch.arange(9.).reshape(3, 3), torch.arange(3.).reshape(1, 3)):
        col = concat_column(v, wp)
        assert tuple(col.shape) == (3, 5) and torch.equal(col[:, :2], v) and torch.equal(col[:, 2:], wp.expand(3, -1))


def test_product_imports_nothing_from_oracle():
    pkg = os.path.join(ROOT, '3d-fm-gan_amd')
    seen = 0
    for d, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith('.py'):
                continue
            seen += 1
            with open(os.path.join(d, f)) as fh:
                tree = ast.parse(fh.read())
            for node in ast.walk(tree):
                names = ([a.name for a in node.names] if isinstance(node, ast.Import)
                         else [node.module or ''] if isinstance(node, ast.ImportFrom) else [])
                assert not any(n.split('.')[0] == 'oracle' for n in names), (f, names)
    assert seen > 40
