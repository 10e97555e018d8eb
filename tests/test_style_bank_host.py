"""CPU tests of the style bank's boundary and of the re-animation fixture: the new symbols are declared and exported,
the table layout is pinned, bad arguments are refused before any HIP call, the public re-animation entry points have
no CPU path, and tests/golden/reanimate.npz agrees with the CPU oracle run with the photo repeated."""
import os
import re

import numpy as np
import pytest
import torch

import reanimate_cases
import synth
from nets import lib
from test_oracle_golden import _img_close, _sd_from_manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('fmgan_style_bank_entry_bytes', 'fmgan_style_bank_f32', 'fmgan_demod_bank_f32')


def test_style_bank_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'fmgan_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    L = lib()
    for n in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % n, hdr), f'{n} is not declared in include/fmgan_hip.h'
        assert hasattr(L, n), f'{n} is not exported'
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for n in SYMBOLS:
        assert n in doc, f'{n} is not described in INTEGRATION.md'


def test_style_bank_entry_layout_is_pinned():
    from op import style_bank
    assert lib().fmgan_style_bank_entry_bytes() == style_bank._ENTRY.itemsize
    style_bank._check_layout()
    # pointers first, then the 64-bit offsets, then the 32-bit fields: no padding anywhere
    assert style_bank._ENTRY.itemsize == sum(style_bank._ENTRY[n].itemsize for n in style_bank._ENTRY.names)


def test_style_bank_refuses_bad_arguments_without_gpu():
    L = lib()
    p = 4096    # any non-null address: every check below fails before a pointer is used or a HIP call is made
    ok = dict(table=p, n=3, w=p, wplus=p, wb=1, batch=3, d=512, out=p)

    def style(**kw):
        a = dict(ok, **kw)
        return L.fmgan_style_bank_f32(a['table'], a['n'], a['w'], a['wplus'], a['wb'], a['batch'], a['d'], a['out'], None)

    for name in ('table', 'w', 'wplus', 'out'):
        assert style(**{name: None}) == -1, name
    assert style(n=0) == -1 and style(d=0) == -1 and style(batch=-1) == -1 and style(d=-4) == -1
    assert style(wb=2, batch=3) == -1 and style(wb=0) == -1
    assert style(batch=0) == 0 and style(batch=0, wb=0) == 0

    def demod(table=p, n=3, styles=p, batch=3, out=p):
        return L.fmgan_demod_bank_f32(table, n, styles, batch, out, None)

    assert demod(table=None) == -1 and demod(styles=None) == -1 and demod(out=None) == -1
    assert demod(n=0) == -1 and demod(batch=-1) == -1
    assert demod(batch=0) == 0


def _generator():
    import stylegan2
    return stylegan2.Generator(32, 512, 1, generator_net_shape=[8, 8, 8, 8, 8, 8, 6, 6]).eval()


def test_reanimation_has_no_cpu_path():
    from Util.network_util import Encode_Photo, Forward_Inference_Reanimate, PhotoCode, Reanimate_From_Codes
    G = _generator()

    def never(x):
        raise AssertionError('an encoder ran on a CPU tensor')

    photo = torch.zeros(1, 3, 256, 256)
    with pytest.raises(RuntimeError):
        Encode_Photo(photo, never, never)
    code = PhotoCode(torch.zeros(1, G.n_latent, 512), torch.zeros(1, 8, 4, 4))
    with pytest.raises(RuntimeError):
        Forward_Inference_Reanimate(code, torch.zeros(2, 3, 256, 256), never, never, G)
    with pytest.raises(RuntimeError):
        Reanimate_From_Codes(code, torch.zeros(2, 512), None, G, randomize_noise=False)
    with torch.no_grad(), pytest.raises(RuntimeError):
        G(None, use_external_input_tensor=True, external_input_tensor=torch.zeros(2, 8, 4, 4),
          comod=(torch.zeros(2, 512), torch.zeros(1, G.n_latent, 512), None))


def test_comod_is_rejected_outside_the_plain_inference_forward():
    G = _generator()
    comod = (torch.zeros(2, 512), torch.zeros(1, G.n_latent, 512), None)
    tsr = torch.zeros(2, 8, 4, 4)
    kw = dict(use_external_input_tensor=True, external_input_tensor=tsr, comod=comod)
    with torch.no_grad():
        for bad in (dict(PPL_regularize=True), dict(return_latents=True), dict(return_style_scalars=True)):
            with pytest.raises(ValueError):
                G(None, **kw, **bad)
        with pytest.raises(ValueError):
            G(None, comod=comod)                                        # no external tensor
        with pytest.raises(ValueError):
            G(None, use_external_input_tensor=True, comod=comod)
    with pytest.raises(ValueError):
        G(None, **kw)                                                   # grad mode


def test_sliced_columns_and_comod_column():
    """The one statement of the co-modulation rule that the pipelined, the serial and the per-layer forward share."""
    from op.style_bank import comod_column, sliced_columns
    assert sliced_columns(None, 10, 18) == frozenset(range(10))
    assert sliced_columns(None, 14, 10) == frozenset(range(10))
    assert sliced_columns([-1, 0, 3, 9, 10, 99], 10, 10) == frozenset({0, 3, 9})
    assert sliced_columns(range(2, 20), 18, 10) == frozenset(range(2, 10))
    assert sliced_columns([], 10, 10) == frozenset()
    assert isinstance(sliced_columns([1], 10, 10), frozenset)
    w = synth.tensor('comod/w', (3, 16))
    for wp in (synth.tensor('comod/wp3', (3, 10, 16)), synth.tensor('comod/wp1', (1, 10, 16))):
        sliced = sliced_columns([0, 3, 4, 12], 10, wp.shape[1])
        for i in range(wp.shape[1]):
            col = comod_column(w, wp[:, i], i, sliced)
            assert tuple(col.shape) == (3, 16)
            if i in (0, 3, 4):
                assert torch.equal(col, w * wp[:, i]), i
            else:
                assert torch.equal(col, w), i


def test_styled_conv_refuses_a_precomputed_modulation_outside_the_fused_path():
    import stylegan2
    from op.style_bank import Modulation
    layer = stylegan2.StyledConv(8, 6, 3, 16)
    pre = Modulation(torch.ones(2, 8), torch.ones(2, 6))
    msg = 'precomputed styles serve the fused inference path on float32 GPU tensors only'
    with torch.enable_grad(), pytest.raises(RuntimeError, match=msg):
        layer(torch.zeros(2, 8, 4, 4), pre)
    with torch.no_grad(), pytest.raises(RuntimeError, match=msg):       # no_grad, but not on the GPU
        layer(torch.zeros(2, 8, 4, 4), pre)


def test_style_bank_starts_without_table_after_deepcopy():
    import copy
    from op.style_bank import StyleBank
    G = _generator()
    G._style_bank = StyleBank(G)
    G._style_bank._source, G._style_bank._tables, G._style_bank._buffers = object(), {'x': 1}, {2: None}
    H = copy.deepcopy(G)
    assert H._style_bank is not G._style_bank and H._style_bank.root is H
    assert H._style_bank._source is None and not H._style_bank._tables and not H._style_bank._buffers
    assert [c for c, _ in H._style_bank.layers()][0] is H.conv1.conv
    assert [col for _, col in G._style_bank.layers()] == [0, 1, 1, 2, 3, 3, 4, 5, 5, 6, 7]


@pytest.mark.parametrize('c', reanimate_cases.REANIMATE_CASES, ids=lambda c: c['name'])
def test_reanimate_fixture_matches_oracle_with_photo_repeated(c, golden):
    """The reference ran frame by frame with the one photo; the oracle runs one batch with the photo repeated.  Gate of
    test_oracle_golden.py::test_e2e_oracle (5e-4 of the image's max on the sample and the statistics)."""
    from oracle import torch_oracle as T
    g = golden('reanimate')
    man = golden.manifest('encoders')
    n_latent = int(np.log2(c['size'])) * 2 - 2
    sd_tsr = _sd_from_manifest('resnet', man['resnet'], 5)
    sd_w = _sd_from_manifest('resnet', man['resnet'], 6)
    sd_wp = _sd_from_manifest('psp', man[f'psp{n_latent}'], 7)
    sd_g = _sd_from_manifest('generator', golden.manifest('generator')['g256_full'], 4)
    p, r = reanimate_cases.inputs(c)
    with torch.no_grad():
        img = T.forward_inference_3_encoder(p.expand(c['frames'], -1, -1, -1).contiguous(), r, sd_tsr, sd_w, sd_wp, sd_g,
                                            c['size'], c['tsr_encode'], c['sliced_layer'], c['use_tanh'])
    assert tuple(img.shape) == (c['frames'], 3, c['size'], c['size'])
    assert g[c['name'] + '/sub'].shape == g[c['name'] + '/sub64'].shape == (c['frames'], 3, 32, 32)
    assert g[c['name'] + '/sub64'].dtype == np.float64
    _img_close(img, g, c['name'], c['stride'], rel=5e-4)
