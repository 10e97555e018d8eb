"""GPU tests of the re-animation path: the style bank's two kernels against the per-layer launches they replace (bits),
the Generator with `comod=` against the plain forward (bits), live weights, reference parity of Encode_Photo +
Forward_Inference_Reanimate and of the chunked driver against tests/golden/reanimate.npz, graph capture, and the GIF
driver."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import cases
import reanimate_cases
import synth
from gpumem import dev, guarded, guards_intact
from nets import encoders, load
from parity import img_close

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ bank kernels alone
BANK_SHAPES = [(6, 3), (64, 64), (96, 48), (512, 512), (576, 32)]     # (cin, cout): cout 3 -> a partial 4-wave block,
#                                                                        cin 576 -> the uncached demod branch


def _bank_layers(style_dim, slicing):
    """Synthetic entries: the five shapes demodulated (3x3-like) + one undemodulated (ToRGB-like, no wsq, no bias)."""
    layers = []
    for j, (cin, cout) in enumerate(BANK_SHAPES + [(64, 3)]):
        rgb = j == len(BANK_SHAPES)
        n = f'bank/{style_dim}/{j}'
        layers.append(dict(
            ws=synth.tensor(n + '/ws', (cin, style_dim), scale=style_dim ** -0.5).to(dev()),
            bs=None if rgb else synth.tensor(n + '/bs', (cin,), scale=0.1, shift=1.0).to(dev()),
            wsq=None if rgb else synth.tensor(n + '/wsq', (cout, cin)).square().to(dev()),
            col=(3 * j + 1) % 7, sliced=dict(mixed=j % 2 == 0, all=True, none=False)[slicing],
            cout=cout, scale=1.0 / (3.0 * cin ** 0.5), eps=1e-8, demodulate=not rgb))
    return layers


@pytest.mark.parametrize('slicing', ['mixed', 'all', 'none'])
@pytest.mark.parametrize('shared', [True, False], ids=['P1', 'PT'])
@pytest.mark.parametrize('T', [1, 3, 65])
@pytest.mark.parametrize('style_dim', [40, 512])
def test_bank_kernels_equal_the_per_layer_launches(style_dim, T, shared, slicing):
    """fmgan_style_bank_f32 / fmgan_demod_bank_f32 on synthetic entries: torch.equal to fmgan_equal_linear_f32 on the
    explicitly multiplied column and fmgan_modconv_demod_wsq_f32 on the wsq buffer; every output element written, no guard
    word touched, two launches identical, and each style within (K+2) * 2^-24 * sum|w*x| of its float64 value (K fma
    roundings of a K-term sum in any order, one for the product W*W+, one for the bias add)."""
    from op import _native
    from op.style_bank import Table
    n_styles = 7
    layers = _bank_layers(style_dim, slicing)
    table = Table(layers, n_styles)
    w = synth.tensor(f'bank/w/{T}', (T, style_dim)).to(dev())
    wp = synth.tensor(f'bank/wp/{T}', (1 if shared else T, n_styles, style_dim)).to(dev())
    ns, nd = T * table.style_floats, T * table.demod_floats
    assert table.style_floats == sum(c for c, _ in BANK_SHAPES) + 64 and table.demod_floats == sum(o for _, o in BANK_SHAPES)
    sbuf, styles = guarded(ns)
    dbuf, demod = guarded(nd)
    table.run(w, wp, styles, demod)
    first = (styles.clone(), demod.clone())
    assert guards_intact(sbuf) and guards_intact(dbuf)
    assert not torch.isnan(styles).any() and not torch.isnan(demod).any()
    table.run(w, wp, styles, demod)
    assert torch.equal(styles, first[0]) and torch.equal(demod, first[1])
    assert guards_intact(sbuf) and guards_intact(dbuf)
    views = table.views(T, styles, demod)
    for l, (s, d) in zip(layers, views):
        x = (w * wp[:, l['col']]) if l['sliced'] else w
        ref_s = _native.equal_linear(x.contiguous(), l['ws'], l['bs'])
        assert torch.equal(s, ref_s), (l['ws'].shape, 'style')
        if l['demodulate']:
            cout, cin = l['wsq'].shape
            ref_d = _native.modconv_demod(torch.empty(cout, cin, 3, 3, device='meta'), ref_s, l['scale'], l['eps'], l['wsq'])
            assert torch.equal(d, ref_d), (l['ws'].shape, 'demod')
        else:
            assert d is None
        w64, x64 = l['ws'].double(), x.double()                         # x is the fp32 product: its rounding is in K+2
        exact = x64 @ w64.T + (0 if l['bs'] is None else l['bs'].double())
        bound = (style_dim + 2) * 2.0 ** -24 * (x64.abs() @ w64.abs().T)
        assert bool(((s.double() - exact).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ Generator bits
def _narrow_g():
    import stylegan2
    c = cases.GENERATOR_CASES[0]
    return load(stylegan2.Generator(c['size'], 512, c['n_mlp'], generator_net_shape=c['shape']), 'generator', 4)


def _codes(G, T, P, cin0, tag):
    w = synth.tensor(f'{tag}/w/{T}', (T, 512)).to(dev())
    wp = synth.tensor(f'{tag}/wp/{T}/{P}', (P, G.n_latent, 512), scale=0.5, shift=1.0).to(dev())
    tsr = synth.tensor(f'{tag}/tsr/{T}/{P}', (P, cin0, 4, 4)).to(dev())
    return w, wp, tsr


def _plain(G, w, wp, tsr, sliced, **noise_kw):
    """The forward as it was before: the latent built by the caller, the tensor repeated."""
    T = w.shape[0]
    n = wp.shape[1]
    sl = set(range(n)) if sliced is None else set(sliced)
    latent = torch.stack([w * wp[:, i] if i in sl else w for i in range(n)], 1)
    with torch.no_grad():
        return G(None, latent_styles=[latent], input_is_latent=True, use_external_input_tensor=True,
                 external_input_tensor=tsr.expand(T, -1, -1, -1).contiguous(), **noise_kw)


@contextlib.contextmanager
def _count_bank_launches():
    """Counts the calls of the two bank bindings inside the block."""
    from op import _native
    n = {'style_bank': 0, 'demod_bank': 0}
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


def _three_ways(G, w, wp, tsr, sliced, **noise_kw):
    import stylegan2
    from Util.network_util import PhotoCode, Reanimate_From_Codes
    code = PhotoCode(wp, tsr)
    prev = stylegan2.STYLE_BANK
    try:
        stylegan2.STYLE_BANK = True
        with _count_bank_launches() as n:
            bank = Reanimate_From_Codes(code, w, None, G, sliced_layer=sliced, **noise_kw).clone()
        # the bank, not a per-layer fall-back, served that forward: one launch pair, from this Generator's own table
        sb = G._style_bank
        assert n == {'style_bank': 1, 'demod_bank': 1}
        assert sb is not None and sb._tables and w.shape[0] in sb._buffers and sb._source is G._live_weights._table
        assert all(t.n == len(sb.layers()) == 2 + 3 * len(G.to_rgbs) for t in sb._tables.values())
        stylegan2.STYLE_BANK = False
        with _count_bank_launches() as n:
            per_layer = Reanimate_From_Codes(code, w, None, G, sliced_layer=sliced, **noise_kw).clone()
        assert n == {'style_bank': 0, 'demod_bank': 0}
    finally:
        stylegan2.STYLE_BANK = prev
    return bank, per_layer, _plain(G, w, wp, tsr, sliced, **noise_kw)


@pytest.mark.parametrize('T', [1, 3, 8])
@pytest.mark.parametrize('P', ['shared', 'per_frame'])
def test_generator_comod_bits_narrow(T, P):
    G = _narrow_g()
    w, wp, tsr = _codes(G, T, 1 if P == 'shared' else T, 16, 'gbits')
    for sliced in (None, [0, 3, 4, 9]):
        bank, per_layer, plain = _three_ways(G, w, wp, tsr, sliced, randomize_noise=False)
        assert tuple(plain.shape) == (T, 3, 64, 64)
        assert torch.equal(bank, plain) and torch.equal(per_layer, plain)
    # explicit noise planes [1,1,H,W]
    noise = [synth.tensor(f'gbits/noise{i}', tuple(getattr(G.noises, f'noise_{i}').shape)).to(dev())
             for i in range(G.num_layers)]
    bank, per_layer, plain = _three_ways(G, w, wp, tsr, None, noise=noise)
    assert torch.equal(bank, plain) and torch.equal(per_layer, plain)
    assert not torch.equal(plain, _plain(G, w, wp, tsr, None, randomize_noise=False))


def test_generator_latent_columns_bits_narrow():
    """W+ handed over one column at a time is the W+ tensor, bit for bit (the pipelined forward is compared to a
    tolerance only because its encoders are not reproducible; the Generator is), each column asked for in layer order."""
    G = _narrow_g()
    lat = synth.tensor('gcols/lat', (3, G.n_latent, 512)).to(dev())
    tsr = synth.tensor('gcols/tsr', (3, 16, 4, 4)).to(dev())
    kw = dict(use_external_input_tensor=True, external_input_tensor=tsr, randomize_noise=False)
    asked = []

    def column(i):
        asked.append(i)
        return lat[:, i]
    with torch.no_grad():
        tensor = G(None, latent_styles=[lat], input_is_latent=True, **kw)
        columns = G(None, latent_columns=column, **kw)
    assert tuple(tensor.shape) == (3, 3, 64, 64) and torch.equal(columns, tensor)
    assert asked == [0, 1] + [i + j for i in range(1, G.n_latent - 1, 2) for j in range(3)]


def test_generator_comod_bits_full_256():
    """Generator(256, 512, 8) at T = 2: a Winograd layer (16^2..128^2 x >= 256 channels) and the fused RGB epilogue at
    the last resolution are on the path."""
    import stylegan2
    G = load(stylegan2.Generator(256, 512, 8), 'generator', 4)
    with torch.no_grad():
        assert stylegan2.winograd_pays(2, 512, 512, 32, 32)
        assert G.convs[-1].rgb_fusable((2, 0, 256, 256), torch.empty(1, device=dev()))
    w, wp, tsr = _codes(G, 2, 1, 512, 'gbits256')
    bank, per_layer, plain = _three_ways(G, w, wp, tsr, list(range(4, 14)), randomize_noise=False)
    assert torch.equal(bank, plain) and torch.equal(per_layer, plain)
    # more style columns than the generator has layers, as in the pipelined path
    wp18 = torch.cat([wp, synth.tensor('gbits256/extra', (1, 4, 512)).to(dev())], 1)
    bank18, _, _ = _three_ways(G, w, wp18, tsr, list(range(4, 18)), randomize_noise=False)
    assert torch.equal(bank18, plain)
    # random noise: runs, and differs
    from Util.network_util import PhotoCode, Reanimate_From_Codes
    rnd = Reanimate_From_Codes(PhotoCode(wp, tsr), w, None, G)
    assert tuple(rnd.shape) == (2, 3, 256, 256) and bool(torch.isfinite(rnd).all()) and not torch.equal(rnd, plain)
    # under autocast: fp32 with autocast off
    with torch.autocast('cuda', dtype=torch.bfloat16):
        ac = Reanimate_From_Codes(PhotoCode(wp, tsr), w, None, G, sliced_layer=list(range(4, 14)), randomize_noise=False)
    assert ac.dtype == torch.float32 and torch.equal(ac, plain)


def test_comod_refuses_other_dtypes_and_shapes():
    from Util.network_util import PhotoCode, Reanimate_From_Codes
    G = _narrow_g()
    w, wp, tsr = _codes(G, 3, 1, 16, 'refuse')
    with pytest.raises(RuntimeError):
        Reanimate_From_Codes(PhotoCode(wp.double(), tsr), w, None, G, randomize_noise=False)
    with pytest.raises(ValueError):
        Reanimate_From_Codes(PhotoCode(wp[:, :3], tsr), w, None, G, randomize_noise=False)        # n_styles < n_latent
    with pytest.raises(ValueError):
        Reanimate_From_Codes(PhotoCode(wp.expand(2, -1, -1), tsr), w, None, G, randomize_noise=False)   # P not in {1, T}


# ------------------------------------------------------------------------------------------------ live weights
def test_comod_reads_live_weights_and_survives_deepcopy():
    G = _narrow_g()
    w, wp, tsr = _codes(G, 3, 1, 16, 'live')
    a, _, plain_a = _three_ways(G, w, wp, tsr, None, randomize_noise=False)
    assert torch.equal(a, plain_a)
    G.convs[0].conv.modulation.weight.data.mul_(1.5)
    G.to_rgb1.conv.modulation.bias.data.add_(0.25)
    b, per_layer_b, plain_b = _three_ways(G, w, wp, tsr, None, randomize_noise=False)
    assert not torch.equal(b, a)
    assert torch.equal(b, plain_b) and torch.equal(per_layer_b, plain_b)
    H = copy.deepcopy(G)
    assert H._style_bank is not G._style_bank and H._style_bank._source is None
    H.conv1.conv.modulation.weight.data.mul_(0.5)
    c, _, plain_c = _three_ways(H, w, wp, tsr, None, randomize_noise=False)
    assert torch.equal(c, plain_c) and not torch.equal(c, b)
    b2, _, _ = _three_ways(G, w, wp, tsr, None, randomize_noise=False)
    assert torch.equal(b2, b)                                            # the original still uses its own parameters
    # LiveWeights rebuilds onto the same parameter addresses (as after A -> B -> A): its pointer key is unchanged, its
    # buffers are new, and the bank must follow them
    old_table = G._style_bank._source
    G._live_weights._key = None
    G.convs[1].conv.modulation.weight.data.mul_(0.75)
    d, _, plain_d = _three_ways(G, w, wp, tsr, None, randomize_noise=False)
    assert G._live_weights._table is not old_table and G._style_bank._source is G._live_weights._table
    assert torch.equal(d, plain_d) and not torch.equal(d, b)


# ------------------------------------------------------------------------------------------------ reference parity
@pytest.fixture(scope='module')
def nets256():
    import stylegan2
    return encoders(14) + (load(stylegan2.Generator(256, 512, 8), 'generator', 4),)


def _gate(img, g, c):
    """The project's end-to-end gate (test_hip_models.py: 5e-5 of the image's max, the float64 companion, the stats)."""
    img_close(img.detach().float().cpu().numpy(), g[c['name'] + '/sub'], g[c['name'] + '/stats'], c['stride'],
              g[c['name'] + '/sub64'], 5e-5)


@pytest.mark.parametrize('c', reanimate_cases.REANIMATE_CASES, ids=lambda c: c['name'])
def test_reanimate_golden(c, golden, nets256):
    from Util.network_util import Encode_Photo, Forward_Inference_Reanimate
    e_tsr, e_w, e_wp, G = nets256
    p, r = (t.to(dev()) for t in reanimate_cases.inputs(c))
    code = Encode_Photo(p, e_tsr, e_wp, c['tsr_encode'])
    assert tuple(code.w_plus.shape) == (1, 14, 512)
    assert (code.tensor is None) == (c['tsr_encode'] == 'Render Image')
    if code.tensor is not None:
        assert tuple(code.tensor.shape) == (1, 512, 4, 4)
    img = Forward_Inference_Reanimate(code, r, e_tsr, e_w, G, tsr_encode=c['tsr_encode'], sliced_layer=c['sliced_layer'],
                                      use_tanh=c['use_tanh'], randomize_noise=False)
    assert tuple(img.shape) == (c['frames'], 3, 256, 256)
    _gate(img, golden('reanimate'), c)


def test_reanimate_frames_chunked_golden(golden, nets256):
    """reanim_256 through the driver in chunks of 2 + 1: every frame, in order, passes the gate against the fixture, and
    the uint8 frames are tensor2im_batch of the float frames."""
    from Evaluation.visual_eval import Reanimate_Frames, tensor2im_batch
    c = reanimate_cases.REANIMATE_CASES[0]
    g = golden('reanimate')
    p, r = (t.to(dev()) for t in reanimate_cases.inputs(c))
    e_tsr, e_w, e_wp, G = nets256
    images, floats = Reanimate_Frames(p, r, (e_tsr, e_w, e_wp, G), chunk=2, return_float=True, tsr_encode=c['tsr_encode'],
                                      sliced_layer=c['sliced_layer'], use_tanh=c['use_tanh'], randomize_noise=False)
    assert len(images) == 3 and tuple(floats.shape) == (3, 3, 256, 256)
    _gate(floats, g, c)
    scale = float(np.abs(g[c['name'] + '/sub']).max())
    for t in range(3):                                                   # frame order: each frame against ITS reference frame
        a = floats[t].cpu().numpy()[..., ::c['stride'], ::c['stride']]
        np.testing.assert_allclose(a, g[c['name'] + '/sub'][t], atol=5e-5 * scale, rtol=5e-5)
        assert images[t].dtype == np.uint8 and images[t].shape == (256, 256, 3)
    np.testing.assert_array_equal(np.stack(images), tensor2im_batch(floats).cpu().numpy())
    # a list of [3,H,W] frames is the same input
    again = Reanimate_Frames(p, list(r), (e_tsr, e_w, e_wp, G), chunk=3, tsr_encode=c['tsr_encode'], randomize_noise=False)
    assert len(again) == 3 and all(x.shape == (256, 256, 3) for x in again)


# ------------------------------------------------------------------------------------------------ graph capture
def test_reanimate_from_codes_graph_capture_equals_eager():
    from Util.hip_graph import GraphedForward
    from Util.network_util import PhotoCode, Reanimate_From_Codes
    G = _narrow_g()
    w, wp, tsr = _codes(G, 3, 1, 16, 'graph')
    noise = [synth.tensor(f'graph/noise{i}', tuple(getattr(G.noises, f'noise_{i}').shape)).to(dev())
             for i in range(G.num_layers)]
    code = PhotoCode(wp, tsr)

    def fwd(w_):
        return Reanimate_From_Codes(code, w_, None, G, noise=noise)

    eager = fwd(w).clone()
    gg = GraphedForward(fwd, (w,))
    for _ in range(3):
        assert torch.equal(gg(w), eager)
    w2 = synth.tensor('graph/w2', (3, 512)).to(dev())
    eager2 = fwd(w2).clone()
    assert not torch.equal(eager2, eager)
    assert torch.equal(gg(w2), eager2)


# ------------------------------------------------------------------------------------------------ GIF driver
class _FixedEncoder(torch.nn.Module):
    """Pooled image -> code through one fixed matrix, on deterministic kernels: the library convolutions of the real
    encoders are not bit-reproducible run to run (profiles/r02_determinism.md), and this test compares two runs bit for
    bit.  out = reshape(mean-pooled image [B, 3*4*4] @ A) * scale + shift."""

    def __init__(self, name, shape, scale, shift):
        super().__init__()
        self.shape, self.scale, self.shift = shape, scale, shift
        self.register_buffer('a', synth.tensor('gif/' + name, (48, int(np.prod(shape)))))

    def forward(self, x):
        pooled = torch.nn.functional.adaptive_avg_pool2d(x, 4).reshape(x.shape[0], 48)
        return ((pooled @ self.a) * self.scale + self.shift).reshape(x.shape[0], *self.shape)


def test_gif_driver_equals_reanimate_frames(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from Evaluation.visual_eval import Get_Single_Photo_Multi_Render_Result, Load_GIF_As_Img_List, Reanimate_Frames
    G = _narrow_g()
    mods = (_FixedEncoder('tsr', (16, 4, 4), 0.5, 0.0).to(dev()), _FixedEncoder('w', (512,), 0.5, 0.0).to(dev()),
            _FixedEncoder('wp', (G.n_latent, 512), 0.2, 1.0).to(dev()), G)
    rng = np.random.Generator(np.random.Philox(key=77))
    photo = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    frames = [np.full((256, 256, 3), 40 + 60 * t, np.uint8) for t in range(3)]       # flat colours survive the GIF palette
    for t, f in enumerate(frames):
        f[32 * t:32 * t + 64, 16:200] = (250, 10 * t, 128)
    Image.fromarray(photo).save(tmp_path / 'photo.png')
    pil = [Image.fromarray(f) for f in frames]
    pil[0].save(tmp_path / 'render.gif', save_all=True, append_images=pil[1:], duration=40, loop=0)

    def transform(img):
        a = torch.from_numpy(np.asarray(img.convert('RGB'), dtype=np.uint8).copy())
        return a.permute(2, 0, 1).float() / 127.5 - 1.0

    loaded = Load_GIF_As_Img_List(str(tmp_path / 'render.gif'), transform)
    assert len(loaded) == 3 and all(tuple(t.shape) == (3, 256, 256) for t in loaded)
    assert not torch.equal(loaded[0], loaded[1]) and not torch.equal(loaded[1], loaded[2])
    out = Get_Single_Photo_Multi_Render_Result(str(tmp_path / 'photo.png'), str(tmp_path / 'render.gif'), mods, transform,
                                               dev(), chunk=2, randomize_noise=False)
    assert len(out) == 3 and all(o.dtype == np.uint8 and o.shape == (64, 64, 3) for o in out)
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])
    p = transform(Image.open(tmp_path / 'photo.png')).unsqueeze(0).to(dev())
    ref = Reanimate_Frames(p, torch.stack(loaded).to(dev()), mods, chunk=2, randomize_noise=False)
    for a, b in zip(out, ref):
        np.testing.assert_array_equal(a, b)
