"""GPU tests of the 2-encoder scheme: the concatenating style-bank kernel against the per-layer launches it replaces
(bits), the Generator with `comod_concat=` (and `comod=` on its ConstantInput) against the plain forward (bits),
reference parity of Forward_Inference in its four modes and of the re-animation pair against tests/golden/two_encoder.npz,
and the scheme under autograd (every parameter gradient of the three modules, and the in-forward path lengths)."""
import contextlib

import numpy as np
import pytest
import torch

import cases
import synth
import test_hip_train as tht            # the gradient rule's constants (MARGIN, FLOOR*, KINK_*); no test is taken from it
import two_encoder_cases as tc
from gpumem import dev, guarded, guards_intact
from nets import PinNoise, load
from parity import img_close

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ bank kernel alone
BANK_SHAPES = [(6, 3), (64, 64), (96, 48), (512, 512), (576, 32)]     # (cin, cout), as tests/test_reanimate.py
# Dv odd: no alignment of the W+ row relative to the lane stride; total under 64: idle lanes; 65: the split in the middle
# of a stride; (512, 512): the product shape
CONCAT_DIMS = [(1, 63), (24, 16), (64, 64), (65, 447), (512, 512)]


def _bank_layers(style_dim, tag):
    """Synthetic entries (copy of tests/test_reanimate.py::_bank_layers): the five shapes demodulated (3x3-like) + one
    undemodulated (ToRGB-like, no wsq, no bias); ws is [cin, style_dim]."""
    layers = []
    for j, (cin, cout) in enumerate(BANK_SHAPES + [(64, 3)]):
        rgb = j == len(BANK_SHAPES)
        n = f'bankcat/{tag}/{j}'
        layers.append(dict(
            ws=synth.tensor(n + '/ws', (cin, style_dim), scale=style_dim ** -0.5).to(dev()),
            bs=None if rgb else synth.tensor(n + '/bs', (cin,), scale=0.1, shift=1.0).to(dev()),
            wsq=None if rgb else synth.tensor(n + '/wsq', (cout, cin)).square().to(dev()),
            col=(3 * j + 1) % 7, sliced=j % 2 == 0,                       # the concatenating kernel ignores `sliced`
            cout=cout, scale=1.0 / (3.0 * cin ** 0.5), eps=1e-8, demodulate=not rgb))
    return layers


@pytest.mark.parametrize('shared', [True, False], ids=['P1', 'PT'])
@pytest.mark.parametrize('T', [1, 3, 65])
@pytest.mark.parametrize('dims', CONCAT_DIMS, ids=lambda d: f'{d[0]}+{d[1]}')
def test_concat_bank_equals_the_per_layer_launches(dims, T, shared):
    """fmgan_style_bank_concat_f32 / fmgan_demod_bank_f32 on synthetic entries: torch.equal to fmgan_equal_linear_f32 on
    the materialised torch.cat([v, wplus[:, col]], 1) and fmgan_modconv_demod_wsq_f32 on it; guard words intact, two
    launches identical, and each style within (K+1) * 2^-24 * sum|w*x| of its float64 value (K fma roundings of a K-term
    sum and one bias add; no product rounding: the concatenation is exact)."""
    from op import _native
    from op.style_bank import Table
    dv, dw = dims
    k, n_styles = dv + dw, 7
    layers = _bank_layers(k, f'{dv}+{dw}')
    table = Table(layers, n_styles)
    assert table.style_dim == k
    v = synth.tensor(f'bankcat/v/{T}', (T, dv)).to(dev())
    wp = synth.tensor(f'bankcat/wp/{T}', (1 if shared else T, n_styles, dw)).to(dev())
    sbuf, styles = guarded(T * table.style_floats)
    dbuf, demod = guarded(T * table.demod_floats)
    table.run_concat(v, wp, styles, demod)
    first = (styles.clone(), demod.clone())
    assert guards_intact(sbuf) and guards_intact(dbuf)
    assert not torch.isnan(styles).any() and not torch.isnan(demod).any()          # every element written
    table.run_concat(v, wp, styles, demod)
    assert torch.equal(styles, first[0]) and torch.equal(demod, first[1])
    assert guards_intact(sbuf) and guards_intact(dbuf)
    for l, (s, d) in zip(layers, table.views(T, styles, demod)):
        x = torch.cat([v, wp[:, l['col']].expand(T, -1)], 1).contiguous()
        ref_s = _native.equal_linear(x, l['ws'], l['bs'])
        assert torch.equal(s, ref_s), (l['ws'].shape, 'style')
        if l['demodulate']:
            cout, cin = l['wsq'].shape
            ref_d = _native.modconv_demod(torch.empty(cout, cin, 3, 3, device='meta'), ref_s, l['scale'], l['eps'], l['wsq'])
            assert torch.equal(d, ref_d), (l['ws'].shape, 'demod')
        else:
            assert d is None
        w64, x64 = l['ws'].double(), x.double()
        exact = x64 @ w64.T + (0 if l['bs'] is None else l['bs'].double())
        bound = (k + 1) * 2.0 ** -24 * (x64.abs() @ w64.abs().T)
        assert bool(((s.double() - exact).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ Generator bits
def _generator(kind):
    """'narrow': GENERATOR_CASES[0]'s widths at style_dim 96 (Dv 32 + Dw 64); 'full': Generator(64, 1024, 8)."""
    import stylegan2
    if kind == 'narrow':
        c = cases.GENERATOR_CASES[0]
        return load(stylegan2.Generator(c['size'], 96, c['n_mlp'], generator_net_shape=c['shape']), 'generator', 4), 32, 16
    return load(stylegan2.Generator(64, 1024, 8), 'generator', 4), 512, 512


@contextlib.contextmanager
def _count_bank_launches():
    """Counts the calls of the bank bindings inside the block (as tests/test_reanimate.py::_count_bank_launches)."""
    from op import _native
    n = {'style_bank': 0, 'style_bank_concat': 0, 'demod_bank': 0}
    orig = {k: getattr(_native, k) for k in n}

    def counted(k):
        def f(*a, **kw):
            n[k] += 1
            return orig[k](*a, **kw)
        return f
    try:
        for k in n:
            setattr(_native, k, counted(k))
        yield n
    finally:
        for k in n:
            setattr(_native, k, orig[k])


@contextlib.contextmanager
def _style_bank(on):
    import stylegan2
    prev = stylegan2.STYLE_BANK
    stylegan2.STYLE_BANK = on
    try:
        yield
    finally:
        stylegan2.STYLE_BANK = prev


@pytest.mark.parametrize('kind', ['narrow', 'full'])
def test_generator_comod_concat_bits(kind):
    """comod_concat= with the bank == with the bank off == the plain latent_styles=[cat] forward, bit for bit; with and
    without an external tensor, P in {1, T}, T in {1, 3}; one concatenating style launch and one demod launch per forward."""
    G, dv, cin0 = _generator(kind)
    dw = G.style_dim - dv
    for T in (1, 3):
        for P in (1, T) if T > 1 else (1,):
            v = synth.tensor(f'gcat/{kind}/v/{T}', (T, dv)).to(dev())
            wp = synth.tensor(f'gcat/{kind}/wp/{T}/{P}', (P, G.n_latent, dw), scale=0.5, shift=1.0).to(dev())
            tsr = synth.tensor(f'gcat/{kind}/tsr/{T}', (T, cin0, 4, 4)).to(dev())
            latent = torch.cat([v.unsqueeze(1).repeat(1, G.n_latent, 1), wp.expand(T, -1, -1)], 2)
            for ext in (dict(use_external_input_tensor=True, external_input_tensor=tsr), {}):
                with torch.no_grad():
                    plain = G(None, latent_styles=[latent], input_is_latent=True, randomize_noise=False, **ext).clone()
                    with _style_bank(True), _count_bank_launches() as n:
                        bank = G(None, comod_concat=(v, wp), randomize_noise=False, **ext).clone()
                    assert n == {'style_bank': 0, 'style_bank_concat': 1, 'demod_bank': 1}
                    sb = G._style_bank
                    assert sb is not None and sb._source is G._live_weights._table and T in sb._buffers
                    assert ('concat', G.n_latent) in sb._tables
                    with _style_bank(False), _count_bank_launches() as n:
                        per_layer = G(None, comod_concat=(v, wp), randomize_noise=False, **ext).clone()
                    assert n == {'style_bank': 0, 'style_bank_concat': 0, 'demod_bank': 0}
                assert tuple(plain.shape) == (T, 3, 64, 64)
                assert torch.equal(bank, plain) and torch.equal(per_layer, plain), (T, P, bool(ext))


def test_generator_comod_on_constant_input_bits():
    """comod= without an external tensor (the 2-encoder 'Multiplication' mode): the plain forward on ConstantInput."""
    G, _, _ = _generator('narrow')
    for T, P in ((1, 1), (3, 1), (3, 3)):
        w = synth.tensor(f'gmul/w/{T}', (T, 96)).to(dev())
        wp = synth.tensor(f'gmul/wp/{T}/{P}', (P, G.n_latent, 96), scale=0.5, shift=1.0).to(dev())
        for sliced in (None, [1, 2, 5]):
            sl = set(range(G.n_latent)) if sliced is None else set(sliced)
            latent = torch.stack([w * wp[:, i] if i in sl else w for i in range(G.n_latent)], 1)
            with torch.no_grad():
                plain = G(None, latent_styles=[latent], input_is_latent=True, randomize_noise=False).clone()
                for on in (True, False):
                    with _style_bank(on), _count_bank_launches() as n:
                        out = G(None, comod=(w, wp, sliced), randomize_noise=False)
                    assert n['style_bank'] == n['demod_bank'] == int(on) and n['style_bank_concat'] == 0
                    assert torch.equal(out, plain), (T, P, sliced, on)


def test_comod_concat_refusals():
    G, dv, cin0 = _generator('narrow')
    T = 3
    v = synth.tensor('gcat/refuse/v', (T, dv)).to(dev())
    wp = synth.tensor('gcat/refuse/wp', (1, G.n_latent, G.style_dim - dv)).to(dev())
    tsr = synth.tensor('gcat/refuse/tsr', (T, cin0, 4, 4)).to(dev())
    kw = dict(randomize_noise=False)
    with pytest.raises(ValueError):
        G(None, comod_concat=(v, wp), **kw)                                                      # grad enabled
    with torch.no_grad():
        G(None, comod_concat=(v, wp), **kw)                                                      # the accepted form
        with pytest.raises(RuntimeError):
            G(None, comod_concat=(v, wp.double()), **kw)                                         # float64 W+
        with pytest.raises(ValueError):
            G(None, comod_concat=(v[:, :-1], wp), **kw)                                          # Dv + Dw != style_dim
        with pytest.raises(ValueError):
            G(None, comod_concat=(v, wp[:, :3]), **kw)                                           # n_styles < n_latent
        with pytest.raises(ValueError):
            G(None, comod_concat=(v, wp.expand(2, -1, -1)), **kw)                                # P not in {1, T}
        with pytest.raises(ValueError):
            G(None, comod_concat=(v, wp), comod=(v, wp, None), **kw)                             # together with comod=
        with pytest.raises(ValueError):
            G(None, comod_concat=(v, wp), latent_columns=lambda i: v, **kw)
        for bad in (dict(PPL_regularize=True), dict(return_latents=True), dict(return_style_scalars=True)):
            with pytest.raises(ValueError):
                G(None, comod_concat=(v, wp), **bad, **kw)
        with pytest.raises(ValueError):
            G(None, comod_concat=(v, wp), use_external_input_tensor=True, external_input_tensor=tsr[:2], **kw)


# ------------------------------------------------------------------------------------------------ reference parity
@pytest.fixture(scope='module')
def built():
    """case -> (tensor encoder, modulation encoder, Generator) on the device, built once per distinct set of modules."""
    import resnet_encoder
    import stylegan2
    from psp_encoder_model.encoders import psp_encoders
    cache = {}

    def get(c):
        key = (c['size'], c['co_mod'] if c['co_mod'] != 'Multiplication' else 'M', tc.uses_psp(c))
        if key not in cache:
            cache[key] = tuple(m.to(dev()) for m in tc.build(c, resnet_encoder, psp_encoders, stylegan2))
        return cache[key]
    yield get
    cache.clear()


@contextlib.contextmanager
def _pipeline(on):
    from Util import network_util
    prev = network_util.PIPELINE
    network_util.PIPELINE = on
    try:
        yield
    finally:
        network_util.PIPELINE = prev


def _gate(img, g, c):
    """The project's end-to-end gates with their defaults (parity.img_close: 1e-4 of the image's max, no farther from
    float64 than the reference's fp32, the stats)."""
    img_close(img.detach().float().cpu().numpy(), g[c['name'] + '/sub'], g[c['name'] + '/stats'], c['stride'],
              g[c['name'] + '/sub64'])


def _forward(c, mods, p, r, mod_encode=None, seen=None):
    """Forward_Inference of a case; `seen` collects the keyword names of every Generator call it makes."""
    from Util.network_util import Forward_Inference
    e_tsr, e_w, G = mods

    def call(**kw):
        if seen is not None:
            seen.append(sorted(k for k, v in kw.items() if v is not None))
        return G(**kw)
    with torch.no_grad():
        return Forward_Inference(p, r, e_tsr, e_w, PinNoise(G, call), mod_encode=mod_encode or c['mod_encode'],
                                 co_modulation=c['co_mod'], sliced_layer=c['sliced_layer'], use_tanh=c['use_tanh'])


@pytest.mark.parametrize('c', tc.FORWARD_CASES, ids=lambda c: c['name'])
def test_forward_inference_golden(c, golden, built):
    """Forward_Inference in its four modes against the reference, on the pipelined schedule and with PIPELINE off; a
    co-modulation mode gives the same image for both mod_encode values, as the reference does."""
    g = golden('two_encoder')
    mods = built(c)
    p, r = (t.to(dev()) for t in tc.inputs(c))
    for on in (True, False):
        seen = []
        with _pipeline(on):
            img = _forward(c, mods, p, r, seen=seen)
        assert tuple(img.shape) == (c['b'], 3, c['size'], c['size'])
        _gate(img, g, c)
        # the schedule under test did run: W+ by columns where the pSp encoder can hand them over, the latent tensor else
        assert len(seen) == 1 and ('latent_columns' in seen[0]) == (on and tc.uses_psp(c)), seen
        assert ('latent_styles' in seen[0]) != ('latent_columns' in seen[0])
    if c['co_mod'] is not None:
        other = [m for m in ('Render Image', 'Photo Image') if m != c['mod_encode']][0]
        _gate(_forward(c, mods, p, r, mod_encode=other), g, c)


@pytest.mark.parametrize('c', tc.REANIMATE_CASES, ids=lambda c: c['name'])
def test_reanimate_2_encoder_golden(c, golden, built):
    """One photo, 3 frames in chunks of 2 + 1 through the driver: every frame, in order, against the reference run frame
    by frame with the one photo; the uint8 frames are tensor2im_batch of the float frames."""
    from Evaluation.visual_eval import Reanimate_Frames_2_Encoder, tensor2im_batch
    from Util.network_util import Encode_Photo_2_Encoder
    g = golden('two_encoder')
    e_tsr, e_w, G = built(c)
    p, r = (t.to(dev()) for t in tc.reanimate_inputs(c))
    code = Encode_Photo_2_Encoder(p, e_tsr, e_w, c['mod_encode'], c['co_mod'])
    if c['co_mod'] is None:
        assert code.latent is None and tuple(code.tensor.shape) == (1, 512, 4, 4)
    else:
        assert code.tensor is None and tuple(code.latent.shape) == (1, 14, 512)
    images, floats = Reanimate_Frames_2_Encoder(p, r, (e_tsr, e_w, G), chunk=2, return_float=True,
                                                mod_encode=c['mod_encode'], co_modulation=c['co_mod'],
                                                sliced_layer=c['sliced_layer'], use_tanh=c['use_tanh'],
                                                randomize_noise=False)
    assert len(images) == 3 and tuple(floats.shape) == (3, 3, 256, 256)
    _gate(floats, g, c)
    sub = g[c['name'] + '/sub']
    scale = float(np.abs(sub).max())
    for t in range(3):                                                   # frame order: each frame against ITS reference frame
        a = floats[t].cpu().numpy()[..., ::c['stride'], ::c['stride']]
        np.testing.assert_allclose(a, sub[t], atol=1e-4 * scale, rtol=1e-4)
        assert images[t].dtype == np.uint8 and images[t].shape == (256, 256, 3)
    np.testing.assert_array_equal(np.stack(images), tensor2im_batch(floats).cpu().numpy())


# ------------------------------------------------------------------------------------------------ autograd
def check_grads(g, prefix, named_params, kinks=None):
    """Every parameter gradient vs the fixture (strided sample + norm): the rule of tests/test_hip_train.py::check_grads
    with its automatic floors — |hip - fp64| <= MARGIN * |ref_fp32 - fp64| + floor * max|fp64|, floor FLOOR_MIOPEN for
    the encoders (prefix e_*), FLOOR for the Generator, FLOOR_SCALAR for one-element tensors; the kink allowance (a
    local, bounded deviation, collected in `kinks`) for encoder tensors only."""
    n = 0
    net = prefix.split('/')[-1]
    encoder = net.startswith('e_')
    floor = tht.FLOOR_MIOPEN if encoder else tht.FLOOR
    for name, p in named_params:
        key = f'{prefix}/{name}'
        if key + '/s' not in g.files:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, f'{key}: reference has no gradient here'
            continue
        assert p.grad is not None, f'{key}: no gradient'
        s, nrm = cases.grad_sample(p.grad)
        s64, n64 = g[key + '/s64'], float(g[key + '/n64'])
        s32, n32 = g[key + '/s'], float(g[key + '/n'])
        scale = max(float(np.abs(s64).max()), 1e-30)
        e_hip = float(np.abs(s - s64).max()) / scale
        e_ref = float(np.abs(s32 - s64).max()) / scale
        en_hip, en_ref = abs(nrm - n64) / max(n64, 1e-30), abs(n32 - n64) / max(n64, 1e-30)
        fl, fn = (tht.FLOOR_SCALAR, tht.FLOOR_SCALAR) if p.numel() == 1 else (floor, tht.FLOOR_NORM)
        print(f'GRAD {key}: sample {e_hip:.3e} (reference {e_ref:.3e})  norm {en_hip:.3e} (reference {en_ref:.3e})')
        over = e_hip > tht.MARGIN * e_ref + fl or en_hip > tht.MARGIN * en_ref + fn
        outliers = int((np.abs(s - s64) / scale > tht.MARGIN * e_ref + fl).sum())
        if (kinks is not None and encoder and over and e_hip <= tht.KINK_MAX
                and en_hip <= tht.MARGIN * en_ref + tht.KINK_NORM and outliers <= tht.KINK_ELEMS):
            kinks.append((key, e_hip, en_hip, outliers))
        else:
            assert e_hip <= tht.MARGIN * e_ref + fl, f'{key}: sample err {e_hip:.3e} vs reference-fp32 err {e_ref:.3e}'
            assert en_hip <= tht.MARGIN * en_ref + fn, f'{key}: norm err {en_hip:.3e} vs reference-fp32 err {en_ref:.3e}'
        n += 1
    return n


def _grad_nets():
    import resnet_encoder
    import stylegan2
    from psp_encoder_model.encoders import psp_encoders
    mods = tuple(m.to(dev()).requires_grad_(True) for m in tc.build(tc.GRAD_CASE, resnet_encoder, psp_encoders, stylegan2))
    return dict(zip(('e_tsr', 'e_w', 'g'), mods))


def test_tensor_transform_forward_backward_golden(golden):
    """'Tensor Transform', B = 2, Generator(64, 1024, 8): image -> L1 -> backward through G and both encoders; image
    and loss as tests/test_hip_train.py::test_cfg3_forward_backward_golden, every fixture gradient compared."""
    from Util.network_util import Forward_Inference
    from Util.training_util import L1_Loss
    g = golden('two_encoder')
    c = tc.GRAD_CASE
    nets = _grad_nets()
    p, r = (t.to(dev()) for t in tc.inputs(c))
    img = Forward_Inference(p, r, nets['e_tsr'], nets['e_w'], PinNoise(nets['g']), mod_encode=c['mod_encode'],
                            co_modulation=c['co_mod'], sliced_layer=c['sliced_layer'], use_tanh=c['use_tanh'])
    loss = L1_Loss(img, tc.target(c).to(dev()))
    loss.backward()
    a = img.detach().cpu().numpy()[..., ::c['stride'], ::c['stride']]
    ref64 = g['grad/img/sub64']
    scale = float(np.abs(ref64).max())
    e_hip, e_ref = np.abs(a - ref64).max() / scale, np.abs(g['grad/img/sub'] - ref64).max() / scale
    print(f'IMAGE |HIP-fp64| {e_hip:.3e}  |reference32-fp64| {e_ref:.3e}  loss {loss.item():.8f} vs {float(g["grad/loss64"]):.8f}')
    assert e_hip <= tht.MARGIN * e_ref + 2e-5, (e_hip, e_ref)
    np.testing.assert_allclose(loss.item(), float(g['grad/loss64']), rtol=2e-5)
    total, kinks, seen = 0, [], []
    for k, m in nets.items():
        total += check_grads(g, 'grad/' + k, m.named_parameters(), kinks=kinks)
        seen += [(k, name, tuple(q.shape)) for name, q in m.named_parameters() if q.grad is not None]
    assert len(kinks) <= tht.KINK_TENSORS, kinks
    assert total == len([k for k in g.files if k.startswith('grad/') and k.endswith('/n64')])   # every fixture tensor visited
    assert ('e_tsr', 'ten_fc.weight', (512, 8192)) in seen
    assert any(k == 'g' and name.endswith('modulation.weight') and shape[1] == 1024 for k, name, shape in seen)
    assert nets['g'].style[1].weight.grad is None                       # mapping network unused (input_is_latent)


def test_path_lengths_and_tanh_on_the_image_only():
    """PPL_regularize=True returns (image [B,3,S,S], path_lengths [B]), both finite; use_tanh bounds the image and leaves
    the path lengths as they are (same probe: the generator's RNG is seeded alike for both runs)."""
    from Util.network_util import Forward_Inference
    c = tc.GRAD_CASE
    nets = _grad_nets()
    p, r = (t.to(dev()) for t in tc.inputs(c))
    outs = {}
    for use_tanh in (False, True):
        torch.manual_seed(11)
        out = Forward_Inference(p, r, nets['e_tsr'], nets['e_w'], PinNoise(nets['g']), mod_encode=c['mod_encode'],
                                co_modulation=c['co_mod'], use_tanh=use_tanh, PPL_regularize=True)
        assert isinstance(out, tuple) and len(out) == 2
        img, pl = out
        assert tuple(img.shape) == (c['b'], 3, c['size'], c['size']) and tuple(pl.shape) == (c['b'],)
        assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(pl).all()) and bool((pl > 0).all())
        outs[use_tanh] = (img.detach(), pl.detach())
        last = pl
    assert float(outs[True][0].abs().max()) <= 1.0 < float(outs[False][0].abs().max())
    # the encoders' library convolutions are not bit-reproducible run to run (1e-6 of their outputs): same path lengths up
    # to that, and the bounded image is tanh of the unbounded one
    torch.testing.assert_close(outs[True][1], outs[False][1], rtol=1e-3, atol=0)
    torch.testing.assert_close(outs[True][0], torch.tanh(outs[False][0]), rtol=0, atol=1e-3)
    last.sum().backward()                                               # differentiable: the regulariser trains through it
    grad = nets['e_tsr'].ten_fc.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
