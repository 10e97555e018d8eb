"""The Winograd transforms' strip kernels (csrc/winograd.hip: one thread per four horizontally adjacent tiles, 16-byte
accesses) and the Winograd weight U of the live-weight refresh (csrc/live_weights.hip).

Every case first asserts the kernel that `_native.wino_select` reports — the launch's own rule: strips where (W/2) % 4 == 0 and
the tensors the launch reads are 16-byte aligned (the output transform: only on rows of at least 32 floats, the shorter rows
measured faster on the tile kernel: profiles/winograd_transforms.md), one tile per thread otherwise — then checks the values
against float64.

Bounds, from the operation counts of csrc/winograd.hip as tests/test_hip_modconv.py derives them (u = 2^-24,
gamma(n) = n u / (1 - n u); a value that passes through n rounded operations carries a relative error of at most gamma(n);
products by 0.5 are exact).  The strip kernels put every element through the same operations in the same order:
  input   v = +-d +-d' (+-d'' +-d''') with d = fl(x * s): one product and two levels of adds on each of 4 terms
          |v - exact| <= gamma(3) * 4 * max|x s|
  output  y = (sum of 9 +-m, four levels of adds) * demod                                  -> 5 operations
          then + fl(nw * noise), + bias, * alpha (negative side), * act_scale              -> 4 more
          |y - exact| <= gamma(5) * 9 max|m| max|demod|                                                        (fuse_act = 0)
          |y - exact| <= gamma(9) * (9 max|m| max|demod| + |nw| max|noise| + max|bias|) * act_scale            (fuse_act = 1)

No shape exists whose column count B*T is no multiple of 4 while W/2 is one: T = (H/2) * (W/2), so (W/2) % 4 == 0 makes T, and
with it every sample's first column b*T and every row of V and M, a multiple of 4 floats.  The rule therefore needs no term
for the columns."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import codeobj
import synth
from gpumem import dev
from nets import load
from parity import tol

pytestmark = pytest.mark.gpu

_U = 2.0 ** -24

# (b, c, h, w): c is cin for the input transform, cout for the output transform
TILE_SHAPES = [(1, 1, 2, 2),       # one tile
               (2, 3, 4, 6)]       # three tiles per row
STRIP_SHAPES = [(1, 5, 8, 16),     # one strip per row: both edge columns padded in the same thread, top and bottom rows too
                (3, 4, 6, 24),     # three strips, h/2 odd
                (2, 2, 4, 40)]     # five strips: left edge, interior, right edge
OFFSET_SHAPE = (1, 3, 8, 16)       # a strip shape on a contiguous view one float into its storage: one tile per thread
# the output transform's strips start at w = 32: the same shapes, then the first two again with rows of 32 and 48 floats
OUT_STRIP_SHAPES = [(1, 5, 8, 32), (3, 4, 6, 48)]


def _sid(s):
    return 'x'.join(map(str, s))


CASES = ([pytest.param(s, False, 'tile', id=_sid(s)) for s in TILE_SHAPES] +
         [pytest.param(s, False, 'strip', id=_sid(s)) for s in STRIP_SHAPES] +
         [pytest.param(OFFSET_SHAPE, True, 'tile', id=_sid(OFFSET_SHAPE) + '_offset4')])
OUT_CASES = ([pytest.param(s, False, 'tile', id=_sid(s)) for s in TILE_SHAPES] +
             [pytest.param(s, False, 'strip' if s[3] >= 32 else 'tile', id=_sid(s)) for s in STRIP_SHAPES + OUT_STRIP_SHAPES] +
             [pytest.param(OFFSET_SHAPE, True, 'tile', id=_sid(OFFSET_SHAPE) + '_offset4'),
              pytest.param(OUT_STRIP_SHAPES[0], True, 'tile', id=_sid(OUT_STRIP_SHAPES[0]) + '_offset4')])


def _gamma(n):
    return n * _U / (1 - n * _U)


def _mats(d):
    bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64, device=d)
    at = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64, device=d)
    return bt, at


def _off4(t):
    """The same values in a contiguous tensor that starts 4 bytes into its storage."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _input_case(shape, offset):
    b, c, h, w = shape
    d = dev()
    x = synth.tensor(f'winofast/in/{shape}/x', shape).to(d)
    s = synth.tensor(f'winofast/in/{shape}/s', (b, c), shift=1.0, scale=0.5).to(d)
    return (_off4(x) if offset else x), s


def _input_ref(x, s):
    b, c, h, w = x.shape
    xs = F.pad(x.double() * s.double()[:, :, None, None], (1, 1, 1, 1))
    tiles = xs.unfold(2, 4, 2).unfold(3, 4, 2)                                    # [b, c, th, tw, 4, 4]
    bt = _mats(x.device)[0]
    ref = torch.einsum('ar,bcyxrq,kq->akcbyx', bt, tiles, bt)                     # Bt d B
    bound = _gamma(3) * 4 * float((x.double() * s.double()[:, :, None, None]).abs().max())
    return ref.reshape(16, c, b * (h // 2) * (w // 2)), bound


@pytest.mark.parametrize('shape,offset,kernel', CASES)
def test_input_transform_vs_float64(shape, offset, kernel):
    from op import _native
    b, c, h, w = shape
    x, s = _input_case(shape, offset)
    assert _native.wino_select('input', b, c, h, w, x) == kernel
    v = _native.wino_input(x, s)
    ref, bound = _input_ref(x, s)
    assert v.shape == ref.shape and torch.isfinite(v).all()
    worst = float((v.double() - ref).abs().max())
    print(f'wino_input {shape} {kernel}: max error {worst:.3e}, bound {bound:.3e}')
    assert worst <= bound, (worst, bound)


# (fuse_act, demod, noise per sample, bias)
VARIANTS = [(True, dm, per, bias) for dm in (True, False) for per in (False, True) for bias in (True, False)] + \
           [(False, True, False, False), (False, False, False, False)]


def _vid(v):
    act, dm, per, bias = v
    if not act:
        return 'noact_' + ('demod' if dm else 'nodemod')
    return '_'.join(['act', 'demod' if dm else 'nodemod', 'noiseB' if per else 'noise1', 'bias' if bias else 'nobias'])


def _output_case(shape, variant, offset=False):
    b, c, h, w = shape
    act, demod, per, with_bias = variant
    d = dev()
    m = synth.tensor(f'winofast/out/{shape}/m', (16, c, b * (h // 2) * (w // 2))).to(d)
    dm = synth.tensor(f'winofast/out/{shape}/dm', (b, c), shift=1.0, scale=0.25).to(d).abs() if demod else None
    noise = synth.tensor(f'winofast/out/{shape}/n', (b if per else 1, 1, h, w)).to(d) if act else None
    bias = synth.tensor(f'winofast/out/{shape}/b', (c,), scale=0.1).to(d) if act and with_bias else None
    nw = torch.tensor([0.3], device=d) if act else None
    return (_off4(m) if offset else m), dm, noise, nw, bias


def _output_ref(m, dm, noise, nw, bias, shape, act, alpha=0.2, act_scale=2 ** 0.5):
    b, c, h, w = shape
    at = _mats(m.device)[1]
    mm = m.double().view(4, 4, c, b, h // 2, w // 2)
    ref = torch.einsum('ja,aqobyx,kq->boyjxk', at, mm, at).reshape(b, c, h, w)      # At M A
    dmax = 1.0
    if dm is not None:
        ref = ref * dm.double()[:, :, None, None]
        dmax = float(dm.abs().max())
    mag = 9 * float(m.abs().max()) * dmax
    if not act:
        return ref, _gamma(5) * mag
    pre = ref + float(nw.double()) * noise.double()
    bmax = 0.0
    if bias is not None:
        pre = pre + bias.double()[None, :, None, None]
        bmax = float(bias.abs().max())
    ref = torch.where(pre > 0, pre, pre * float(np.float32(alpha))) * float(np.float32(act_scale))
    return ref, _gamma(9) * (mag + float(nw) * float(noise.abs().max()) + bmax) * act_scale


@pytest.mark.parametrize('variant', VARIANTS, ids=_vid)
@pytest.mark.parametrize('shape,offset,kernel', OUT_CASES)
def test_output_transform_vs_float64(shape, offset, kernel, variant):
    from op import _native
    b, c, h, w = shape
    act = variant[0]
    m, dm, noise, nw, bias = _output_case(shape, variant, offset)
    assert _native.wino_select('output', b, c, h, w, m, noise) == kernel
    y = _native.wino_output(m, dm, b, h, w, noise=noise, noise_weight=nw, bias=bias, fuse_act=act)
    ref, bound = _output_ref(m, dm, noise, nw, bias, shape, act)
    assert y.shape == ref.shape and torch.isfinite(y).all()
    worst = float((y.double() - ref).abs().max())
    print(f'wino_output {shape} {_vid(variant)} {kernel}: max error {worst:.3e}, bound {bound:.3e}')
    assert worst <= bound, (worst, bound)


def test_select_is_the_launch_rule():
    """Host logic: strips need (w/2) % 4 == 0 and every 16-byte-accessed tensor aligned; sizes the launch refuses raise."""
    from op import _native
    L = _native.lib()
    for out in (0, 1):
        assert L.fmgan_wino_select(out, 8, 512, 64, 64, 1) == 1 and L.fmgan_wino_select(out, 8, 512, 64, 64, 0) == 0
        assert L.fmgan_wino_select(out, 8, 256, 128, 128, 1) == 1 and L.fmgan_wino_select(out, 32, 512, 32, 32, 1) == 1
        assert L.fmgan_wino_select(out, 16, 2048, 18, 30, 1) == 0 and L.fmgan_wino_select(out, 1, 1, 64, 12, 1) == 0
        assert L.fmgan_wino_select(out, 0, 4, 8, 32, 1) == 1
        for bad in ((1, 4, 7, 8), (1, 4, 8, 7), (1, 0, 8, 8), (-1, 4, 8, 8), (1, 4, 0, 8)):
            assert L.fmgan_wino_select(out, *bad, 1) == _native.FMGAN_EINVAL
            with pytest.raises(RuntimeError):
                _native.wino_select(('input', 'output')[out], *bad)
    # rows shorter than 32 floats: strips for the input transform only
    assert [L.fmgan_wino_select(0, 8, 512, 16, w, 1) for w in (8, 16, 24, 32)] == [1, 1, 1, 1]
    assert [L.fmgan_wino_select(1, 8, 512, 16, w, 1) for w in (8, 16, 24, 32)] == [0, 0, 0, 1]
    d = dev()
    m = torch.zeros(16, 3, 64, device=d)
    noise = torch.zeros(1, 1, 8, 32, device=d)
    assert _native.wino_select('output', 1, 3, 8, 32, m, noise) == 'strip'
    assert _native.wino_select('output', 1, 3, 8, 32, m, None) == 'strip'
    assert _native.wino_select('output', 1, 3, 8, 32, m, _off4(noise)) == 'tile'    # a misaligned noise plane alone decides too
    y = _native.wino_output(m, None, 1, 8, 32, noise=_off4(noise + 1), noise_weight=torch.ones(1, device=d), fuse_act=True)
    assert torch.equal(y, torch.full_like(y, 2 ** 0.5))


@pytest.mark.parametrize('shape', STRIP_SHAPES + OUT_STRIP_SHAPES, ids=_sid)
def test_strip_kernels_give_the_tile_kernels_bits(shape):
    """The two kernels of each transform on the same values (the tile kernel forced through a copy that starts 4 bytes into
    its storage): the arithmetic is the same, so the results are the same bits."""
    from op import _native
    b, c, h, w = shape
    x, s = _input_case(shape, False)
    xo = _off4(x)
    assert (_native.wino_select('input', b, c, h, w, x), _native.wino_select('input', b, c, h, w, xo)) == ('strip', 'tile')
    assert torch.equal(_native.wino_input(x, s), _native.wino_input(xo, s))
    for variant in ((True, True, True, True), (True, False, False, False), (False, True, False, False)):
        if w < 32:
            continue                    # one kernel for these rows
        m, dm, noise, nw, bias = _output_case(shape, variant)
        mo = _off4(m)
        assert (_native.wino_select('output', b, c, h, w, m, noise), _native.wino_select('output', b, c, h, w, mo, noise)) == \
            ('strip', 'tile')
        kw = dict(noise=noise, noise_weight=nw, bias=bias, fuse_act=variant[0])
        assert torch.equal(_native.wino_output(m, dm, b, h, w, **kw), _native.wino_output(mo, dm, b, h, w, **kw)), variant


# ------------------------------------------------------------------------------------------------------- the whole form
@pytest.mark.parametrize('act', [False, True], ids=['raw', 'act'])
@pytest.mark.parametrize('cfg', [(2, 8, 8, 8, 16), (1, 4, 12, 6, 24), (2, 8, 12, 4, 32)], ids=_sid)
def test_whole_form_vs_float64_convolution(cfg, act):
    """(b, cin, cout, h, w); the last one has rows long enough for the output transform's strips too."""
    from op import _native
    b, cin, cout, h, w = cfg
    d = dev()
    x = synth.tensor(f'winofast/form/{cfg}/x', (b, cin, h, w))
    wgt = synth.tensor(f'winofast/form/{cfg}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'winofast/form/{cfg}/s', (b, cin), shift=1.0, scale=0.5)
    scale = 1.0 / np.sqrt(cin * 9)
    wq = wgt.double() * scale
    ref = F.conv2d(x.double() * s.double()[:, :, None, None], wq, padding=1)
    ref = ref * torch.rsqrt((s.double() ** 2) @ (wq * wq).sum((2, 3)).t() + 1e-8)[:, :, None, None]
    xd, wd, sd = x.to(d), wgt.to(d), s.to(d)
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    kw = {}
    if act:
        noise = synth.tensor(f'winofast/form/{cfg}/n', (1, 1, h, w))
        bias = synth.tensor(f'winofast/form/{cfg}/b', (cout,))
        pre = ref + float(np.float32(0.3)) * noise.double() + bias.double()[None, :, None, None]
        ref = torch.where(pre > 0, pre, pre * float(np.float32(0.2))) * float(np.float32(2 ** 0.5))
        kw = dict(noise=noise.to(d), noise_weight=torch.tensor([0.3], device=d), bias=bias.to(d), fuse_act=True)
    assert _native.wino_select('input', b, cin, h, w, xd) == 'strip'
    assert _native.wino_select('output', b, cout, h, w, kw.get('noise')) == ('strip' if w >= 32 else 'tile')
    y = _native.modconv2d_winograd(xd, wt, sd, dm, **kw)
    ref = ref.numpy()
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print(f'modconv2d_winograd {cfg} act={act}: max error {err:.3e}, atol {tol(ref)["atol"]:.3e}')
    np.testing.assert_allclose(y.cpu().numpy(), ref, **tol(ref))
    assert torch.equal(_native.modconv2d_winograd(xd, wt, sd, dm, **kw), y)                  # two calls, the same bits
    assert torch.equal(_native.modconv2d_winograd(xd, wt, sd, dm, u=_native.wino_weight(wt), **kw), y)


# ------------------------------------------------------------------------------------------------------- U from the refresh
class _Layers(torch.nn.Module):
    def __init__(self):
        import stylegan2
        super().__init__()
        self.wide = stylegan2.ModulatedConv2d(256, 256, 3, 16)                   # whole 64 x 16 refresh tiles
        self.ragged = stylegan2.ModulatedConv2d(264, 280, 3, 16)                 # partial tiles on both sides
        self.narrow = stylegan2.ModulatedConv2d(128, 256, 3, 16)                 # winograd_pays never names it
        self.up = stylegan2.ModulatedConv2d(256, 256, 3, 16, upsample=True)      # not a plain layer


def _fresh_u(m):
    from op import _native
    with torch.no_grad():
        return _native.wino_weight(_native.modconv_weight_prep(m.weight.detach(), m.scale))


def test_refresh_table_holds_the_winograd_weight_of_the_wide_plain_layers():
    """U of the refresh launch is bit for bit wino_weight(wt) computed outside a live forward; it is handed out only inside
    one; an in-place update through .data (no version bump: the case the refresh exists for) reaches the next forward's U."""
    from op.live_weights import LiveWeights, live_u
    net = load(_Layers(), 'generator', 11)
    lw = LiveWeights(net)
    with torch.no_grad():
        assert live_u(net.wide) is None                                            # no forward running
        with lw.fresh():
            assert lw.active
            for m in (net.wide, net.ragged):
                u = m.wino_weight()
                assert u is not None and u is live_u(m) and u.shape == (16, m.out_channel, m.in_channel)
                assert torch.equal(u, _fresh_u(m))
                assert torch.equal(m._live[1], m.mfma_weight())                    # wt and wsq beside it, as before
            assert net.narrow.wino_weight() is None and net.up.wino_weight() is None
            old = net.ragged.wino_weight().clone()
        assert live_u(net.wide) is None and net.wide.wino_weight() is None
        v0 = net.ragged.weight._version
        net.ragged.weight.data.mul_(0.5).add_(0.01)                                # optimiser / EMA style, in place
        assert net.ragged.weight._version == v0
        with lw.fresh():
            u = net.ragged.wino_weight()
            assert not torch.equal(u, old) and torch.equal(u, _fresh_u(net.ragged))
    with lw.fresh():
        assert net.wide.wino_weight() is None                                      # autograd on: derived on the spot


def test_generator_forward_takes_u_from_the_refresh(monkeypatch):
    """Generator(32) at B = 2 runs its 32^2 plain layer in Winograd form (stylegan2.winograd_pays): with the table's U no
    wino_weight launch is left in the forward, and the image is the same bits as with U derived per call."""
    import stylegan2
    from op import _native
    G = load(stylegan2.Generator(32, 512, 2), 'generator', 31)
    assert stylegan2.winograd_pays(2, 512, 512, 32, 32)
    lat = synth.tensor('winofast/gen/lat', (2, G.n_latent, 512)).to(dev())
    tsr = synth.tensor('winofast/gen/tsr', (2, 512, 4, 4)).to(dev())
    calls = []
    orig = _native.conv.wino_weight
    monkeypatch.setattr(_native.conv, 'wino_weight', lambda wt: calls.append(tuple(wt.shape)) or orig(wt))

    def run():
        with torch.no_grad():
            return G(None, latent_styles=[lat], input_is_latent=True, use_external_input_tensor=True,
                     external_input_tensor=tsr, randomize_noise=False).clone()
    a = run()
    assert calls == []
    monkeypatch.setattr(stylegan2, 'live_u', lambda m: None)
    b = run()
    assert calls == [(512, 9, 512)]
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------- code object
def test_strip_kernels_neither_spill_nor_use_scratch(tmp_path):
    """128 registers keep 4 waves per SIMD in flight, which these HBM-bound kernels need to cover the latency."""
    kernels = codeobj.kernel_notes(tmp_path)
    for needle in ('wino_input_strip_f32', 'wino_output_strip_f32'):
        hits = [k for k in kernels if needle in k]
        assert len(hits) == 1, (needle, hits)
        k = kernels[hits[0]]
        print(f'{needle}: {k}')
        assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0 and k['vgpr'] <= 128, (needle, k)
