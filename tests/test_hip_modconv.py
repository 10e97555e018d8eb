"""GPU parity tests for the modulated convolution / ToRGB kernels and the modules built on them."""
import os

import numpy as np
import pytest
import torch

import cases
import launches
import synth
from gpumem import dev
from nets import load
from parity import tol as _tol, window_check as _window_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('c', cases.MODCONV_CASES, ids=lambda c: c['name'])
def test_modulated_conv_golden(c, golden):
    import stylegan2
    g = golden('modules')
    m = load(stylegan2.ModulatedConv2d(c['cin'], c['cout'], c['k'], 512, demodulate=c['demod'], upsample=c['up']),
             'generator', 1, eval=False)          # here and below the modules stay in training mode, as built
    x = synth.tensor(c['name'] + '/x', (c['b'], c['cin'], c['h'], c['h'])).to(dev())
    w = synth.tensor(c['name'] + '/w', (c['b'], 512)).to(dev())
    ref = g[c['name'] + '/out']
    with torch.no_grad():
        y = m(x, w)
    np.testing.assert_allclose(y.cpu().numpy(), ref, **_tol(ref))
    # the differentiable composite used for the backward graph is the same function
    from op import modconv
    with torch.no_grad():
        s = m.modulation(w)
        yc = modconv.modconv_composite(x, m.weight, s, c['demod'], 1 if c['up'] else 0, m.scale)
        if c['up']:
            yc = m.blur(yc)
    np.testing.assert_allclose(yc.cpu().numpy(), ref, **_tol(ref, 5e-5))


@pytest.mark.parametrize('cfg', [
    # (b, cin, cout, h, w, mode)  — every tile configuration: cout >=96 / >=48 / <48, widths 4..>32, sample packing
    (5, 12, 130, 4, 4, 0), (5, 12, 130, 4, 4, 1), (3, 7, 64, 8, 8, 0), (3, 7, 64, 8, 8, 1),
    (2, 33, 32, 16, 16, 0), (2, 33, 32, 16, 16, 1), (1, 16, 100, 33, 35, 0), (1, 16, 100, 33, 35, 1),
    (2, 8, 50, 70, 40, 0), (2, 8, 50, 70, 40, 1), (1, 40, 20, 64, 64, 0), (1, 40, 20, 64, 64, 1),
    (9, 5, 3, 5, 3, 0), (9, 5, 3, 5, 3, 1),
    # mode 2: stride-2 valid conv (downsample branch; data-gradient of mode 1)
    (5, 12, 130, 9, 9, 2), (3, 7, 64, 17, 17, 2), (2, 33, 32, 33, 33, 2), (1, 16, 100, 67, 71, 2),
    (2, 8, 50, 141, 81, 2), (1, 40, 20, 129, 129, 2), (9, 5, 3, 11, 7, 2), (4, 130, 12, 9, 9, 2),
])
@pytest.mark.parametrize('demod', [True, False])
def test_modconv_kernel_vs_c_oracle(cfg, demod):
    from op import _native
    from oracle import c_oracle
    b, cin, cout, h, w, mode = cfg
    x = synth.tensor(f'mck/{cfg}/x', (b, cin, h, w))
    wgt = synth.tensor(f'mck/{cfg}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'mck/{cfg}/s', (b, cin), shift=1.0, scale=0.5)
    scale = 1.0 / np.sqrt(cin * 9)
    ref = c_oracle.modulated_conv2d(x.numpy(), wgt.numpy(), s.numpy(), mode=mode, demodulate=demod)
    xd, wd, sd = x.to(dev()), wgt.to(dev()), s.to(dev())
    wt = _native.modconv_weight_prep(wd, scale)
    np.testing.assert_allclose(wt.cpu().numpy(), (wgt.numpy() * np.float32(scale)).reshape(cout, cin, 9).transpose(1, 2, 0),
                               atol=0, rtol=0)
    dm = _native.modconv_demod(wd, sd, scale) if demod else None
    if demod:
        dref = 1.0 / np.sqrt(((np.float64(scale) * wgt.numpy()[None].astype(np.float64) *
                               s.numpy()[:, None, :, None, None]) ** 2).sum(axis=(2, 3, 4)) + 1e-8)
        np.testing.assert_allclose(dm.cpu().numpy(), dref, rtol=2e-6, atol=0)
    y = _native.modconv2d(xd, wt, sd, dm, mode)
    np.testing.assert_allclose(y.cpu().numpy(), ref, **_tol(ref))


@pytest.mark.parametrize('cfg', [
    # (batch, cin, cout, h, w, keep_out): cout <= 32 -> 32x128 tile, <= 64 -> 64x128, <= 128 -> 128x128 (two channel waves)
    (2, 32, 32, 64, 64, True), (1, 24, 20, 70, 66, True), (2, 16, 32, 128, 128, False),
    (2, 64, 64, 48, 48, True), (1, 40, 50, 75, 61, False),
    (2, 128, 128, 40, 40, True), (1, 72, 100, 49, 57, False), (3, 16, 128, 32, 32, True),
])
def test_conv_with_torgb_in_epilogue_vs_c_oracle(cfg):
    """fmgan_modconv2d_rgb_f32: StyledConv (conv + noise + bias + lrelu) and the following ToRGB (+ bias + skip) in one
    kernel vs the two C-oracle steps; also against this repo's own two-kernel path."""
    check_conv_with_torgb_in_epilogue(cfg)


def check_conv_with_torgb_in_epilogue(cfg):
    """Body of test_conv_with_torgb_in_epilogue_vs_c_oracle (shared with tests/test_hip_modconv_tiles.py)."""
    from op import _native
    from oracle import c_oracle
    b, cin, cout, h, w, keep = cfg
    assert _native.modconv2d_rgb_fusable(b, cin, cout, h, w)
    x = synth.tensor(f'rgbf/{cfg}/x', (b, cin, h, w))
    wgt = synth.tensor(f'rgbf/{cfg}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'rgbf/{cfg}/s', (b, cin), shift=1.0, scale=0.5)
    noise = synth.tensor(f'rgbf/{cfg}/n', (b, 1, h, w))
    nw = torch.tensor([0.3])
    bias = synth.tensor(f'rgbf/{cfg}/b', (cout,))
    rw = synth.tensor(f'rgbf/{cfg}/rw', (3, cout))
    rs = synth.tensor(f'rgbf/{cfg}/rs', (b, cout), shift=1.0, scale=0.5)
    rb = synth.tensor(f'rgbf/{cfg}/rb', (3,))
    skip = synth.tensor(f'rgbf/{cfg}/k', (b, 3, h, w))
    scale, rscale = 1.0 / np.sqrt(cin * 9), 1.0 / np.sqrt(cout)
    conv = c_oracle.modulated_conv2d(x.numpy(), wgt.numpy(), s.numpy(), mode=0, demodulate=True)
    pre = conv + np.float32(0.3) * noise.numpy() + bias.numpy()[None, :, None, None]
    act = (np.where(pre > 0, pre, pre * np.float32(0.2)) * np.float32(2 ** 0.5)).astype(np.float32)
    rgb_ref = c_oracle.to_rgb(act, rw.numpy(), rs.numpy(), rb.numpy(), skip.numpy())
    d = dev()
    xd, wd, sd = x.to(d), wgt.to(d), s.to(d)
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    out, rgb = _native.modconv2d_rgb(xd, wt, sd, dm, noise.to(d), nw.to(d), bias.to(d), 0.2, 2 ** 0.5, rw.to(d), rs.to(d),
                                     rb.to(d), skip.to(d), rscale, keep_out=keep)
    np.testing.assert_allclose(rgb.cpu().numpy(), rgb_ref, **_tol(rgb_ref))
    two = _native.modconv2d(xd, wt, sd, dm, 0, noise=noise.to(d), noise_weight=nw.to(d), bias=bias.to(d), fuse_act=True)
    if keep:
        # the activation is the same conv (the two-kernel path may sum in split-K order: compare within tolerance)
        np.testing.assert_allclose(out.cpu().numpy(), two.cpu().numpy(), **_tol(act))
        np.testing.assert_allclose(out.cpu().numpy(), act, **_tol(act))
    else:
        assert out is None
    rgb2 = _native.torgb(two, rw.to(d), rs.to(d), rb.to(d), skip.to(d), rscale)
    np.testing.assert_allclose(rgb.cpu().numpy(), rgb2.cpu().numpy(), **_tol(rgb_ref))
    # no skip / no bias
    _, rgb3 = _native.modconv2d_rgb(xd, wt, sd, dm, noise.to(d), nw.to(d), bias.to(d), 0.2, 2 ** 0.5, rw.to(d), rs.to(d),
                                    None, None, rscale, keep_out=False)
    ref3 = c_oracle.to_rgb(act, rw.numpy(), rs.numpy(), None, None)
    np.testing.assert_allclose(rgb3.cpu().numpy(), ref3, **_tol(ref3))


@pytest.mark.parametrize('cfg', [
    # (b, cin, cout, h, w, mode): 32-wide tiles; rows of whole 16-byte groups (the wide patch) and not; several x tiles;
    # Cout ragged against the channel tile (generic stores) and whole (buffer stores); multi-round launches of the
    # transposed conv (thin segments shrunk to the main segment's LDS image)
    (1, 16, 32, 40, 36, 0), (1, 16, 32, 40, 38, 0), (2, 8, 64, 36, 68, 0), (1, 24, 20, 33, 100, 0), (1, 8, 128, 37, 96, 0),
    (1, 16, 32, 40, 36, 1), (1, 16, 32, 40, 38, 1), (2, 8, 64, 20, 68, 1), (1, 24, 20, 19, 52, 1),
    (3, 16, 32, 96, 160, 1), (4, 8, 32, 256, 256, 1), (2, 8, 64, 256, 512, 1), (2, 16, 32, 192, 256, 0),
])
def test_modconv_wide_patch_and_buffer_store_paths_vs_c_oracle(cfg):
    """Round 3's staging and store paths of the fp32 kernel (16-byte patch pieces, buffer-store epilogue, bias / demod / style
    through LDS) against the C oracle, with and without the fused activation; plus their fall-backs: the same tensors at a
    4-byte-misaligned address (4-byte patch pieces) and into a strided, odd-aligned output must give the SAME BITS."""
    from op import _native
    from oracle import c_oracle
    b, cin, cout, h, w, mode = cfg
    x = synth.tensor(f'wide/{cfg}/x', (b, cin, h, w))
    wgt = synth.tensor(f'wide/{cfg}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'wide/{cfg}/s', (b, cin), shift=1.0, scale=0.5)
    scale = 1.0 / np.sqrt(cin * 9)
    ref = c_oracle.modulated_conv2d(x.numpy(), wgt.numpy(), s.numpy(), mode=mode, demodulate=True)
    d = dev()
    xd, wd, sd = x.to(d), wgt.to(d), s.to(d)
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    y = _native.modconv2d(xd, wt, sd, dm, mode)
    np.testing.assert_allclose(y.cpu().numpy(), ref, **_tol(ref))
    # same input one float further (not 16-byte aligned): the 4-byte staging path
    flat = torch.empty(xd.numel() + 1, dtype=torch.float32, device=d)
    xm = flat[1:].view_as(xd)
    xm.copy_(xd)
    assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
    assert torch.equal(_native.modconv2d(xm, wt, sd, dm, mode), y)
    # strided output (the aligned-row layout of the upsampling branch: first element at base + 4 bytes)
    oh, ow = y.shape[2:]
    buf, p0, ps, rs = _native.aligned_rows_buffer(b, cout, oh, ow, 1, d)
    buf.fill_(float('nan'))
    _native.modconv2d(xd, wt, sd, dm, mode, strided_out=(p0, ps, rs))
    assert torch.equal(buf[:, :, 1:1 + ow].reshape(b, cout, oh, ow), y)
    assert torch.isnan(buf[:, :, 0]).all() and torch.isnan(buf[:, :, 1 + ow:]).all()
    if mode == 0:
        noise = synth.tensor(f'wide/{cfg}/n', (1, 1, h, w))
        bias = synth.tensor(f'wide/{cfg}/b', (cout,))
        nw = torch.tensor([0.3])
        pre = ref + np.float32(0.3) * noise.numpy() + bias.numpy()[None, :, None, None]
        act = (np.where(pre > 0, pre, pre * np.float32(0.2)) * np.float32(2 ** 0.5)).astype(np.float32)
        ya = _native.modconv2d(xd, wt, sd, dm, 0, noise=noise.to(d), noise_weight=nw.to(d), bias=bias.to(d), fuse_act=True)
        np.testing.assert_allclose(ya.cpu().numpy(), act, **_tol(act))
        assert torch.equal(_native.modconv2d(xm, wt, sd, dm, 0, noise=noise.to(d), noise_weight=nw.to(d), bias=bias.to(d),
                                             fuse_act=True), ya)


@pytest.mark.parametrize('cfg', [(2, 16, 32, 8, 8), (1, 24, 40, 34, 36), (3, 8, 16, 2, 6), (2, 64, 64, 32, 32), (1, 128, 64, 64, 48),
                                 (2, 7, 5, 10, 4)])
@pytest.mark.parametrize('act', [False, True])
def test_winograd_form_vs_c_oracle(cfg, act):
    """fmgan_wino_{weight,input,output}_f32 + 16 batched GEMMs (Winograd F(2x2,3x3) form of the plain modulated conv) against the
    C oracle at the direct kernel's tolerance, with and without the fused StyledConv epilogue, and against the direct kernel."""
    from op import _native
    from oracle import c_oracle
    b, cin, cout, h, w = cfg
    x = synth.tensor(f'wino/{cfg}/x', (b, cin, h, w))
    wgt = synth.tensor(f'wino/{cfg}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'wino/{cfg}/s', (b, cin), shift=1.0, scale=0.5)
    scale = 1.0 / np.sqrt(cin * 9)
    ref = c_oracle.modulated_conv2d(x.numpy(), wgt.numpy(), s.numpy(), mode=0, demodulate=True)
    d = dev()
    xd, wd, sd = x.to(d), wgt.to(d), s.to(d)
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    kw = {}
    if act:
        noise = synth.tensor(f'wino/{cfg}/n', (1, 1, h, w))
        bias = synth.tensor(f'wino/{cfg}/b', (cout,))
        pre = ref + np.float32(0.3) * noise.numpy() + bias.numpy()[None, :, None, None]
        ref = (np.where(pre > 0, pre, pre * np.float32(0.2)) * np.float32(2 ** 0.5)).astype(np.float32)
        kw = dict(noise=noise.to(d), noise_weight=torch.tensor([0.3], device=d), bias=bias.to(d), fuse_act=True)
    y = _native.modconv2d_winograd(xd, wt, sd, dm, **kw)
    np.testing.assert_allclose(y.cpu().numpy(), ref, **_tol(ref))
    yd = _native.modconv2d(xd, wt, sd, dm, 0, **kw)
    np.testing.assert_allclose(y.cpu().numpy(), yd.cpu().numpy(), **_tol(ref))
    assert torch.equal(_native.modconv2d_winograd(xd, wt, sd, dm, **kw), y)          # bit-reproducible
    with pytest.raises(RuntimeError):
        _native.modconv2d_winograd(xd[:, :, :-1], wt, sd, dm)                          # odd height


# ---------------------------------------------------------------------------------------- Winograd transforms, alone
# The three kernels of csrc/winograd.hip are grid-stride loops over one work item per (sample, channel, 2x2 tile) — or per
# (cout, cin) pair — launched with at most num_CU * 32 blocks of 256 threads.  test_winograd_form_vs_c_oracle stays below
# 10^5 work items: one trip.  Here every kernel gets more than two full trips' worth, at a power-of-two plane and at a
# ragged even one, against a float64 statement of Bt (s.d) B, G g Gt and At M A (+ epilogue) on the same device tensors.
#
# Bounds, derived from the operation counts in csrc/winograd.hip (u = 2^-24, gamma(n) = n u / (1 - n u); a value that passes
# through n rounded operations carries a relative error of at most gamma(n); products by 0.5 are exact):
#   input   v = +-d +-d' (+-d'' +-d''')   with d = fl(x * s): one product and two levels of adds on each of 4 terms
#           |v - exact| <= gamma(3) * 4 * max|x s|
#   weight  u = sum of 9 taps with weights in {1, 1/2, 1/4} whose magnitudes sum to at most 9/4: two adds per stage, two stages
#           |u - exact| <= gamma(4) * 9/4 * max|wt|
#   output  y = (sum of 9 +-m, four levels of adds) * demod                                  -> 5 operations
#           then + fl(nw * noise), + bias, * alpha (negative side), * act_scale              -> 4 more
#           |y - exact| <= gamma(5) * 9 max|m| max|demod|                                                        (fuse_act = 0)
#           |y - exact| <= gamma(9) * (9 max|m| max|demod| + |nw| max|noise| + max|bias|) * act_scale            (fuse_act = 1)
#           (the leaky ReLU is 1-Lipschitz, so a sign decided differently near 0 stays inside the same bound)
_WINO_U = 2.0 ** -24


def _gamma(n):
    return n * _WINO_U / (1 - n * _WINO_U)


def _two_trips():
    """Work items of two full trips of the transforms' capped grid on this device."""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 32 * 256


def _wino_mats(d):
    bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64, device=d)
    g = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64, device=d)
    at = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64, device=d)
    return bt, g, at


@pytest.mark.parametrize('cfg', [(8, 520, 64, 64), (16, 2048, 18, 30)], ids=['b8_c520_64x64', 'b16_c2048_18x30'])
def test_winograd_input_transform_past_two_grid_trips_vs_float64(cfg):
    from op import _native
    b, c, h, w = cfg
    th, tw = h // 2, w // 2
    assert b * c * th * tw > _two_trips()
    d = dev()
    gen = torch.Generator(device=d).manual_seed(77)
    x = torch.randn(b, c, h, w, device=d, generator=gen)
    s = 1.0 + 0.5 * torch.randn(b, c, device=d, generator=gen)
    v = _native.wino_input(x, s)
    bt = _wino_mats(d)[0]
    bound = _gamma(3) * 4 * float((x.double() * s.double()[:, :, None, None]).abs().max())
    worst = 0.0
    for b0 in range(0, b, 4):                       # float64 reference a few samples at a time (memory)
        xs = torch.nn.functional.pad(x[b0:b0 + 4].double() * s[b0:b0 + 4].double()[:, :, None, None], (1, 1, 1, 1))
        tiles = xs.unfold(2, 4, 2).unfold(3, 4, 2)                                    # [b, c, th, tw, 4, 4]
        ref = torch.einsum('ar,bcyxrq,kq->akcbyx', bt, tiles, bt)                     # Bt d B
        nb = tiles.shape[0]
        got = v.view(4, 4, c, b, th, tw)[:, :, :, b0:b0 + nb]
        assert torch.isfinite(got).all()
        worst = max(worst, float((got.double() - ref).abs().max()))
        del xs, tiles, ref
    print(f'wino_input {cfg}: max error {worst:.3e}, bound {bound:.3e}')
    assert worst <= bound, (worst, bound)


def test_winograd_weight_transform_past_two_grid_trips_vs_float64():
    from op import _native
    cin, cout = 2050, 2056
    assert cin * cout > _two_trips()
    d = dev()
    gen = torch.Generator(device=d).manual_seed(78)
    wt = torch.randn(cin, 9, cout, device=d, generator=gen)
    u = _native.wino_weight(wt)
    g = _wino_mats(d)[1]
    taps = wt.double().permute(0, 2, 1).reshape(cin, cout, 3, 3)
    ref = torch.einsum('ar,iorq,kq->akoi', g, taps, g).reshape(16, cout, cin)     # G g Gt
    bound = _gamma(4) * 9 / 4 * float(wt.abs().max())
    assert torch.isfinite(u).all()
    worst = float((u.double() - ref).abs().max())
    print(f'wino_weight {cin}x{cout}: max error {worst:.3e}, bound {bound:.3e}')
    assert worst <= bound, (worst, bound)


@pytest.mark.parametrize('variant', ['noise_per_sample', 'noise_shared', 'no_act', 'no_demod'])
@pytest.mark.parametrize('cfg', [(8, 520, 64, 64), (16, 2048, 18, 30)], ids=['b8_c520_64x64', 'b16_c2048_18x30'])
def test_winograd_output_transform_past_two_grid_trips_vs_float64(cfg, variant):
    from op import _native
    b, c, h, w = cfg
    th, tw = h // 2, w // 2
    assert b * c * th * tw > _two_trips()
    d = dev()
    gen = torch.Generator(device=d).manual_seed(79)
    m = torch.randn(16, c, b * th * tw, device=d, generator=gen)
    dm = None if variant == 'no_demod' else 0.5 + torch.rand(b, c, device=d, generator=gen)
    act = variant != 'no_act'
    noise = torch.randn(1 if variant == 'noise_shared' else b, 1, h, w, device=d, generator=gen) if act else None
    nw = torch.tensor([0.3], device=d)
    bias = 0.1 * torch.randn(c, device=d, generator=gen)
    alpha, act_scale = 0.2, 2 ** 0.5
    y = _native.wino_output(m, dm, b, h, w, noise=noise, noise_weight=nw if act else None, bias=bias if act else None,
                            fuse_act=act, alpha=alpha, act_scale=act_scale)
    at = _wino_mats(d)[2]
    mm = m.double().view(4, 4, c, b, th, tw)
    ref = torch.einsum('ja,aqobyx,kq->boyjxk', at, mm, at).reshape(b, c, h, w)      # At M A
    dmax = 1.0
    if dm is not None:
        ref = ref * dm.double()[:, :, None, None]
        dmax = float(dm.max())
    mag = 9 * float(m.abs().max()) * dmax
    if act:
        pre = ref + float(nw.double()) * noise.double() + bias.double()[None, :, None, None]
        ref = torch.where(pre > 0, pre, pre * float(np.float32(alpha))) * float(np.float32(act_scale))
        bound = _gamma(9) * (mag + float(nw) * float(noise.abs().max()) + float(bias.abs().max())) * act_scale
    else:
        bound = _gamma(5) * mag
    assert torch.isfinite(y).all()
    worst = float((y.double() - ref).abs().max())
    print(f'wino_output {cfg} {variant}: max error {worst:.3e}, bound {bound:.3e}')
    assert worst <= bound, (worst, bound)


def test_rgb_fusable_is_host_logic_and_unsupported_shapes_are_refused():
    from op import _native
    assert _native.modconv2d_rgb_fusable(8, 32, 32, 1024, 1024) and _native.modconv2d_rgb_fusable(8, 64, 64, 512, 512)
    assert _native.modconv2d_rgb_fusable(8, 128, 128, 256, 256)
    assert not _native.modconv2d_rgb_fusable(8, 256, 256, 128, 128)      # two output-channel tiles
    assert not _native.modconv2d_rgb_fusable(1, 512, 512, 4, 4)          # tiny layer: small tiles, 16 channel tiles
    x = torch.zeros(1, 256, 128, 128, device=dev())
    wt = torch.zeros(256, 9, 256, device=dev())
    s = torch.ones(1, 256, device=dev())
    with pytest.raises(RuntimeError):
        _native.modconv2d_rgb(x, wt, s, None, None, None, None, 0.2, 1.0, torch.zeros(3, 256, device=dev()), s, None,
                              None, 1.0)


@pytest.mark.parametrize('c', cases.STYLEDCONV_CASES, ids=lambda c: c['name'])
def test_styled_conv_golden_fused_and_unfused(c, golden):
    import stylegan2
    g = golden('modules')
    m = load(stylegan2.StyledConv(c['cin'], c['cout'], 3, 512, upsample=c['up']), 'generator', 2, eval=False)
    oh = c['h'] * 2 if c['up'] else c['h']
    x = synth.tensor(c['name'] + '/x', (c['b'], c['cin'], c['h'], c['h'])).to(dev())
    w = synth.tensor(c['name'] + '/w', (c['b'], 512)).to(dev())
    nz = synth.tensor(c['name'] + '/noise', (c['nb'], 1, oh, oh)).to(dev())
    ref = g[c['name'] + '/out']
    with torch.no_grad():
        y_fused = m(x, w, noise=nz)                      # conv-epilogue / one-pass fused path
    y_graph = m(x, w, noise=nz)                          # autograd path: three separate ops
    np.testing.assert_allclose(y_fused.cpu().numpy(), ref, **_tol(ref))
    np.testing.assert_allclose(y_graph.detach().cpu().numpy(), ref, **_tol(ref))
    # (the two paths share every kernel but the modulation linear: the inference path's matrix-vector kernel and the BLAS
    # GEMM of the autograd path add in different orders, so the style vector differs in its last bit)
    torch.testing.assert_close(y_fused, y_graph.detach(), atol=5e-6, rtol=1e-5)


@pytest.mark.parametrize('c', cases.TORGB_CASES, ids=lambda c: c['name'])
def test_to_rgb_golden(c, golden):
    import stylegan2
    g = golden('modules')
    m = load(stylegan2.ToRGB(c['cin'], 512, upsample=c['skip']), 'generator', 3, eval=False)
    x = synth.tensor(c['name'] + '/x', (c['b'], c['cin'], c['h'], c['h'])).to(dev())
    w = synth.tensor(c['name'] + '/w', (c['b'], 512)).to(dev())
    skip = synth.tensor(c['name'] + '/skip', (c['b'], 3, c['h'] // 2, c['h'] // 2)).to(dev()) if c['skip'] else None
    ref = g[c['name'] + '/out']
    with torch.no_grad():
        y = m(x, w, skip)
    np.testing.assert_allclose(y.cpu().numpy(), ref, **_tol(ref))


@pytest.mark.parametrize('cfg', [(2, 512, 4, 4, True), (3, 40, 8, 8, False), (2, 64, 32, 32, True), (1, 32, 256, 256, True),
                                 (2, 17, 16, 20, True), (8, 32, 512, 512, False)])
def test_torgb_backward_kernel_vs_float64_autograd(cfg):
    """fmgan_torgb_backward_f32 (data gradient + pixel contraction in one pass) through ToRGBFunction.backward: all five
    gradients vs float64 autograd of the differentiable composite (stylegan2.py:389-404 restated); two runs bit-equal."""
    from op import modconv
    b, cin, h, w, with_skip = cfg
    d = dev()
    x = synth.tensor(f'tb/{cfg}/x', (b, cin, h, w)).to(d).requires_grad_(True)
    wgt = synth.tensor(f'tb/{cfg}/w', (1, 3, cin, 1, 1)).to(d).requires_grad_(True)
    s = synth.tensor(f'tb/{cfg}/s', (b, cin), shift=1.0, scale=0.5).to(d).requires_grad_(True)
    bias = synth.tensor(f'tb/{cfg}/b', (1, 3, 1, 1)).to(d).requires_grad_(True)
    skip = synth.tensor(f'tb/{cfg}/k', (b, 3, h, w)).to(d).requires_grad_(True) if with_skip else None
    go = synth.tensor(f'tb/{cfg}/go', (b, 3, h, w)).to(d)
    scale = 1.0 / np.sqrt(cin)
    ins = [x, wgt, s, bias] + ([skip] if with_skip else [])
    assert _native_serves(b, cin, h * w)
    g1 = torch.autograd.grad(modconv.to_rgb(x, wgt, s, bias, skip, scale), ins, go)
    g2 = torch.autograd.grad(modconv.to_rgb(x, wgt, s, bias, skip, scale), ins, go)
    for a, c in zip(g1, g2):
        assert torch.equal(a, c)
    ins64 = [t.detach().double().requires_grad_(True) for t in ins]
    y64 = modconv._torgb_composite(ins64[0], ins64[1], ins64[2], ins64[3], ins64[4] if with_skip else None, scale)
    ref = torch.autograd.grad(y64, ins64, go.double())
    for name, a, r in zip(('x', 'weight', 'style', 'bias', 'skip'), g1, ref):
        err = float((a.double() - r).abs().max() / r.abs().max().clamp_min(1e-30))
        assert err < 2e-5, (name, err)


def _native_serves(b, cin, hw):
    from op import _native
    return _native.lib().fmgan_torgb_backward_splits(b, cin, hw) > 0


def test_torgb_kernel_vs_c_oracle_ragged():
    from op import _native
    from oracle import c_oracle
    for (b, cin, h, w) in ((2, 37, 5, 7), (1, 512, 4, 4), (3, 64, 32, 32), (1, 32, 128, 128)):
        x = synth.tensor(f'rgbk/{cin}{h}/x', (b, cin, h, w))
        wgt = synth.tensor(f'rgbk/{cin}{h}/w', (3, cin))
        s = synth.tensor(f'rgbk/{cin}{h}/s', (b, cin), shift=1.0, scale=0.5)
        bias = synth.tensor(f'rgbk/{cin}{h}/b', (3,))
        skip = synth.tensor(f'rgbk/{cin}{h}/k', (b, 3, h, w))
        ref = c_oracle.to_rgb(x.numpy(), wgt.numpy(), s.numpy(), bias.numpy(), skip.numpy())
        y = _native.torgb(x.to(dev()), wgt.to(dev()), s.to(dev()), bias.to(dev()), skip.to(dev()), 1.0 / np.sqrt(cin))
        np.testing.assert_allclose(y.cpu().numpy(), ref, **_tol(ref))


# ---------------------------------------------------------------------------------------- ToRGB above 128^2, directly
# fmgan_torgb_f32 (csrc/torgb.hip) has three kernels: torgb_small_f32 up to 128 x 128 pixels (the shapes above), and beyond
# that the grid-stride kernel torgb_f32<4> (16-byte loads: H*W a multiple of 4 and in / out / skip 16-byte aligned) or
# torgb_f32<1>.  Its grid is capped at ceil(16 * compute units / batch) blocks of 256 pixel groups per sample.  The C oracle
# (oracle/fmgan_oracle.c, oracle_to_rgb_f32) sums the fp32 products in double.
def _torgb_inputs(cfg, cout=3):
    b, cin, h, w = cfg
    tag = f'rgbl/{cfg}/{cout}'
    return (synth.tensor(tag + '/x', (b, cin, h, w)), synth.tensor(tag + '/w', (cout, cin)),
            synth.tensor(tag + '/s', (b, cin), shift=1.0, scale=0.5), synth.tensor(tag + '/b', (cout,)),
            synth.tensor(tag + '/k', (b, cout, h, w)))


def _torgb_vs_c_oracle(cfg, cout=3, with_bias=True, with_skip=True):
    from op import _native
    from oracle import c_oracle
    x, wgt, s, bias, skip = _torgb_inputs(cfg, cout)
    bias, skip = bias if with_bias else None, skip if with_skip else None
    ref = c_oracle.to_rgb(x.numpy(), wgt.numpy(), s.numpy(), None if bias is None else bias.numpy(),
                          None if skip is None else skip.numpy())
    d = dev()
    args = [t if t is None else t.to(d) for t in (x, wgt, s, bias, skip)]
    assert cfg[2] * cfg[3] > 128 * 128 and all(t is None or t.data_ptr() % 16 == 0 for t in args)
    y = _native.torgb(*args, 1.0 / np.sqrt(cfg[1]))
    assert tuple(y.shape) == (cfg[0], cout, cfg[2], cfg[3]) and y.data_ptr() % 16 == 0
    np.testing.assert_allclose(y.cpu().numpy(), ref, **_tol(ref))
    return y, args


@pytest.mark.parametrize('cout,with_bias,with_skip', [(3, True, True), (1, True, True), (2, True, True), (4, True, True),
                                                      (3, False, True), (3, True, False), (3, False, False)])
def test_torgb_large_image_scalar_kernel_vs_c_oracle(cout, with_bias, with_skip):
    """129 x 129: above 128^2 and H*W = 16641 is no multiple of 4 -> torgb_f32<1>; every output-channel count, with and
    without bias and skip."""
    cfg = (2, 5, 129, 129)
    assert cfg[2] * cfg[3] % 4 != 0
    _torgb_vs_c_oracle(cfg, cout, with_bias, with_skip)


def test_torgb_large_image_vector_kernel_vs_c_oracle_and_its_misaligned_fallback():
    """132 x 128: H*W a multiple of 4, aligned tensors -> torgb_f32<4>.  The same call with `skip` one float into a larger
    buffer is the other half of the predicate -> torgb_f32<1>: the same fused multiply-adds in the same channel order, the
    same two rounded adds, so the same bits."""
    from op import _native
    from gpumem import misaligned
    cfg = (2, 5, 132, 128)
    assert cfg[2] * cfg[3] % 4 == 0
    y, (x, wgt, s, bias, skip) = _torgb_vs_c_oracle(cfg)
    off = misaligned(skip)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert torch.equal(_native.torgb(x, wgt, s, bias, off, 1.0 / np.sqrt(cfg[1])), y)


def test_torgb_large_image_second_trip_of_the_grid_stride_loop_vs_c_oracle():
    """Batch 64 at 129 x 129: the grid cap ceil(16 * CUs / 64) (64 blocks on 256 compute units) is below the
    ceil(16641 / 256) = 66 blocks that would give each thread one pixel, so the first threads take a second trip."""
    cfg = (64, 2, 129, 129)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-16 * cus // cfg[0]) < -(-cfg[2] * cfg[3] // 256), cus
    _torgb_vs_c_oracle(cfg)


def test_weight_prep_layouts():
    from op import _native
    w = synth.tensor('wprep/w', (20, 12, 3, 3))
    wd = w.to(dev())
    k0 = _native.modconv_weight_prep(wd, 0.5, 0).cpu().numpy()
    k1 = _native.modconv_weight_prep(wd, 0.5, 1).cpu().numpy()
    k2 = _native.modconv_weight_prep(wd, 0.5, 2).cpu().numpy()
    wn = (w.numpy() * np.float32(0.5)).reshape(20, 12, 9)
    np.testing.assert_array_equal(k0, wn.transpose(1, 2, 0))
    np.testing.assert_array_equal(k1, wn[:, :, ::-1].transpose(0, 2, 1))
    np.testing.assert_array_equal(k2, wn.transpose(0, 2, 1))


@pytest.mark.parametrize('shape', [(20, 12, 3), (64, 520, 3), (3, 32, 1), (130, 600, 3)])
def test_demod_from_cached_wsq_is_bit_identical(shape):
    """fmgan_modconv_wsq_f32 + fmgan_modconv_demod_wsq_f32 (what inference uses, wsq cached with the weight) must give
    the bits of fmgan_modconv_demod_f32, and both match the float64 closed form."""
    from op import _native
    cout, cin, k = shape
    w = synth.tensor(f'wsq/{cout}x{cin}/w', (cout, cin, k, k))
    s = synth.tensor(f'wsq/{cout}x{cin}/s', (3, cin))
    scale = 1.0 / np.sqrt(cin * k * k)
    wd, sdv = w.to(dev()), s.to(dev())
    direct = _native.modconv_demod(wd, sdv, scale)
    wsq = _native.modconv_wsq(wd)
    cached = _native.modconv_demod(wd, sdv, scale, wsq=wsq)
    assert torch.equal(direct, cached)
    ref = 1.0 / np.sqrt((scale * scale) * (s.double().numpy() ** 2) @ (w.double().numpy() ** 2).sum((2, 3)).T + 1e-8)
    np.testing.assert_allclose(cached.cpu().numpy(), ref, rtol=2e-6)


@pytest.mark.parametrize('cfg', [(2, 6, 10, 5, False, True), (2, 6, 10, 5, True, True), (3, 20, 136, 8, False, True),
                                 (3, 20, 136, 8, True, True), (1, 9, 70, 20, True, False), (2, 16, 8, 16, False, False),
                                 (2, 40, 70, 32, False, True), (1, 33, 65, 40, False, True), (3, 8, 8, 24, False, True)])
def test_first_order_backward_on_hip_vs_oracle(cfg, monkeypatch):
    """loss.backward() without create_graph: data gradient on the MFMA kernel (swapped-role weight layouts, stride-2
    mode for the transposed conv), weight gradient + demodulation chain rule; vs float64 autograd through the CPU
    oracle's weight-modulated grouped conv (the reference's formulation)."""
    # Every configuration has cin <= 40: ModulatedConv2dFunction.backward asks for the weight gradient with fast_only=True,
    # which declines fewer than 48 channels on either side, so all nine take MIOpen's weight gradient whatever HIP_WGRAD says
    # (the backward on this repo's weight-gradient kernel: test_first_order_backward_on_own_wgrad_kernel_vs_oracle below).
    # monkeypatch restores the product default afterwards (round 2 assigned the module attribute and left it at 0 for
    # every later test of the process)
    check_first_order_backward(cfg, 1 if cfg[3] % 8 == 0 else 0, monkeypatch)


def check_first_order_backward(cfg, hip_wgrad, monkeypatch, down=False):
    """Body of the two first-order backward tests; returns the recorder of the launch brackets begun during backward."""
    import stylegan2
    from oracle import torch_oracle as T
    from op import modconv as _mc
    b, cin, cout, h, up, demod = cfg
    monkeypatch.setattr(_mc, 'HIP_WGRAD', hip_wgrad)
    m = stylegan2.ModulatedConv2d(cin, cout, 3, 512, demodulate=demod, upsample=up, downsample=down)
    m.load_state_dict(synth.state_dict('generator', m.state_dict(), seed=21))
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    m = m.to(dev())
    tag = f'bw/{cfg}/down' if down else f'bw/{cfg}'
    x = synth.tensor(tag + '/x', (b, cin, h, h))
    w = synth.tensor(tag + '/w', (b, 512))
    xo, wo = x.double().requires_grad_(True), w.double().requires_grad_(True)
    wt_o, mw_o, mb_o = (sd[k].clone().requires_grad_(True) for k in ('weight', 'modulation.weight', 'modulation.bias'))
    yo = T.modulated_conv2d(xo, wo, wt_o, mw_o, mb_o, demod, up, [1, 3, 3, 1], downsample=down)
    go = synth.tensor(tag + '/go', yo.shape)
    ref = torch.autograd.grad(yo, (xo, wo, wt_o, mw_o, mb_o), go.double())
    xd, wd = x.to(dev()).requires_grad_(True), w.to(dev()).requires_grad_(True)
    yd = m(xd, wd)
    with launches.observed() as obs:
        yd.backward(go.to(dev()))                 # no graph requested -> HIP first-order path
    got = (xd.grad, wd.grad, m.weight.grad, m.modulation.weight.grad, m.modulation.bias.grad)
    for name, g, r in zip(('x', 'latent', 'weight', 'mod.weight', 'mod.bias'), got, ref):
        r = r.numpy()
        np.testing.assert_allclose(g.cpu().numpy(), r, atol=2e-4 * max(1e-6, float(np.abs(r).max())), rtol=2e-4,
                                   err_msg=name)
    return obs


@pytest.mark.parametrize('hip_wgrad', ['own', 0], ids=['own_kernel', 'miopen'])
@pytest.mark.parametrize('cfg,down,setting,bracket,plan', [
    # (b, cin, cout, h, upsample, demodulate), downsample, the HIP_WGRAD that puts the layer on this repo's kernel, the
    # launch bracket (b, cin, cout, conv input h, w, mode) that must then be begun, and its (family, TW, SP, vec)
    ((2, 48, 64, 16, False, True), False, 1, (2, 48, 64, 16, 16, 0), (64, 16, 1, True)),     # d and scale ride in the kernel
    ((1, 64, 48, 16, False, False), False, 1, (1, 64, 48, 16, 16, 0), (64, 16, 1, True)),    # demodulate=False: d = None
    ((2, 50, 70, 17, False, True), False, 1, (2, 50, 70, 17, 17, 0), (64, 16, 1, False)),    # ragged channels, scalar staging
    ((1, 48, 48, 16, True, True), False, 2, (1, 48, 48, 16, 16, 1), (64, 16, 2, True)),      # transposed conv, go 33 x 33
    # downsample: the 4-tap blur with pad (2, 2) makes the 32 x 32 input 33 x 33, the stride-2 conv's input; its backward
    # is the DenseConv family's (mode 2 takes the composite form), whose weight gradient passes demod = None, scale 1
    ((1, 48, 48, 32, False, True), True, 2, (1, 48, 48, 33, 33, 2), (64, 16, 2, True)),
], ids=['plain_demod', 'plain_no_demod', 'plain_ragged', 'upsample', 'downsample'])
def test_first_order_backward_on_own_wgrad_kernel_vs_oracle(cfg, down, setting, bracket, plan, hip_wgrad, monkeypatch):
    """The body of test_first_order_backward_on_hip_vs_oracle at >= 48 channels on both sides, where the module's backward
    takes this repo's weight-gradient kernel: the demodulation and the scale riding in the kernel (or d = None), the
    demodulation's chain-rule term added on top, modes 1 and 2 under HIP_WGRAD = 2.  The bracket of the expected launch must
    have been begun, on the kernel the library's own plan names; under HIP_WGRAD = 0 (MIOpen's weight gradient, same
    reference, same bound) none may be."""
    from op import _native
    b, cin, cout, h, w, mode = bracket
    family, tw, sp, _ks, _tps, _ntiles, vec = _native.modconv_wgrad_select(b, cin, cout, h, w, mode)
    assert (family, tw, sp, vec) == plan
    obs = check_first_order_backward(cfg, setting if hip_wgrad == 'own' else 0, monkeypatch, down=down)
    assert obs.infos('modconv_wgrad') == ([bracket] if hip_wgrad == 'own' else []), obs.seen


def test_dense_conv_wgrad_under_create_graph_runs_own_kernel_without_demod(monkeypatch):
    """DenseConvWgrad (the weight gradient of the create_graph=True path) at cin = cout = 48: op.modconv._wgrad hands the
    kernel demod = None, a style of ones and scale 1.  First order against float64 autograd of F.conv2d on the CPU at the
    weight-gradient kernels' bound (tests/test_hip_modconv_wgrad.py), and one derivative further — through the graph the
    Function recorded — at test_dense_conv_family_differentiates_into_itself's bound for that order."""
    from op import _native, modconv
    import torch.nn.functional as F
    monkeypatch.setattr(modconv, 'HIP_WGRAD', 1)
    b, cin, cout, h, w = 2, 48, 48, 8, 16
    assert _native.modconv_wgrad_select(b, cin, cout, h, w, 0)[:3] == (64, 16, 1)
    u = synth.tensor('dcw/u', (b, cin, h, w))
    wt = synth.tensor('dcw/w', (cout, cin, 3, 3), scale=0.3)
    g1 = synth.tensor('dcw/g1', (b, cout, h, w))

    def chain(conv, uu, ww, g):
        gu, gw = torch.autograd.grad(conv(uu, ww), (uu, ww), g, create_graph=True)
        hu, = torch.autograd.grad(gw.pow(2).mean(), uu)                  # d/du of G_0(u, g): a data gradient with weight dL/dgw
        return gw.detach().cpu().double(), hu.cpu().double()

    gw_o, hu_o = chain(lambda a, c: F.conv2d(a, c, padding=1), u.double().requires_grad_(True),
                       wt.double().requires_grad_(True), g1.double())
    with launches.observed() as obs:
        gw_d, hu_d = chain(lambda a, c: modconv.DenseConv.apply(a, c, 0), u.to(dev()).requires_grad_(True),
                           wt.to(dev()).requires_grad_(True), g1.to(dev()))
    assert obs.infos('modconv_wgrad') == [(b, cin, cout, h, w, 0)], obs.seen
    torch.testing.assert_close(gw_d, gw_o, atol=2e-5 * float(gw_o.abs().max()), rtol=2e-5)
    torch.testing.assert_close(hu_d, hu_o, atol=1e-4 * float(hu_o.abs().max()), rtol=1e-3)


@pytest.mark.parametrize('shape', [
    # (b, cin, cout, h, w): 32 x 32-tile kernel (< 48 channels) and 64 x 64-tile kernel (TW = 32 / 16, ragged sizes,
    # partial channel tiles, odd heights, widths that are no multiple of the tile)
    (2, 64, 96, 64, 64), (1, 32, 32, 128, 128), (3, 100, 50, 17, 33), (8, 512, 512, 16, 16), (2, 64, 64, 64, 64),
    (1, 128, 64, 40, 48), (4, 70, 130, 33, 20), (1, 48, 200, 9, 16), (2, 256, 256, 128, 128)])
def test_wgrad_kernel_vs_fp64(shape):
    """fmgan_modconv_wgrad_f32 vs a float64 conv weight gradient of the same (d*go, s*x) on the GPU."""
    from op import _native
    b, cin, cout, h, w = shape
    go = synth.tensor(f'wg/{shape}/go', (b, cout, h, w)).to(dev())
    x = synth.tensor(f'wg/{shape}/x', (b, cin, h, w)).to(dev())
    s = synth.tensor(f'wg/{shape}/s', (b, cin), shift=1.0, scale=0.5).to(dev())
    d = synth.tensor(f'wg/{shape}/d', (b, cout), shift=1.0, scale=0.3).to(dev())
    gw = _native.modconv_wgrad(go, d, x, s, 0.37)
    ref = torch.nn.grad.conv2d_weight((x * s[:, :, None, None]).double(), (cout, cin, 3, 3),
                                      (go * d[:, :, None, None]).double(), padding=1) * 0.37
    torch.testing.assert_close(gw.double(), ref, atol=2e-5 * float(ref.abs().max()), rtol=2e-5)
    gw2 = _native.modconv_wgrad(go, d, x, s, 0.37)
    assert torch.equal(gw, gw2)          # fixed-order split over pixels: bit-reproducible


def test_downsample_branch_on_hip_vs_composite():
    """ModulatedConv2d(downsample=True) (stylegan2.py:281-286; unused by the Generator, kept for API parity): blur then
    the stride-2 MFMA mode vs the PyTorch-ROCm composite."""
    import stylegan2
    from op import modconv
    m = stylegan2.ModulatedConv2d(12, 20, 3, 512, downsample=True)
    m.load_state_dict(synth.state_dict('generator', m.state_dict(), seed=22))
    m = m.to(dev())
    x = synth.tensor('ds/x', (2, 12, 16, 16)).to(dev())
    w = synth.tensor('ds/w', (2, 512)).to(dev())
    with torch.no_grad():
        y = m(x, w)
        s = m.modulation(w)
        ref = modconv.modconv_composite(m.blur(x), m.weight, s, True, 2, m.scale)
    assert tuple(y.shape) == (2, 20, 8, 8)
    torch.testing.assert_close(y, ref, atol=2e-5 * float(ref.abs().max()), rtol=1e-5)


def test_modconv_gradients_match_reference_formulation():
    """First and second derivatives through the HIP forward (recompute-composite backward) equal autograd through
    the CPU oracle's weight-modulated grouped conv (the reference's formulation)."""
    import stylegan2
    from oracle import torch_oracle as T
    for up in (False, True):
        m = load(stylegan2.StyledConv(6, 10, 3, 512, upsample=up), 'generator', 11, eval=False)
        sd = {'m.' + k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        x = synth.tensor(f'mcg/{up}/x', (2, 6, 5, 5))
        w = synth.tensor(f'mcg/{up}/w', (2, 512))
        oh = 10 if up else 5
        nz = synth.tensor(f'mcg/{up}/n', (2, 1, oh, oh))
        xo, wo = x.double().requires_grad_(True), w.double().requires_grad_(True)
        yo = T.styled_conv(sd, 'm', xo, wo, nz.double(), up)
        go = synth.tensor(f'mcg/{up}/go', yo.shape)
        gxo, gwo = torch.autograd.grad(yo, (xo, wo), go.double(), create_graph=True)
        pen_o = gxo.pow(2).sum() + gwo.pow(2).sum()
        ggo, = torch.autograd.grad(pen_o, wo)
        xd, wd = x.to(dev()).requires_grad_(True), w.to(dev()).requires_grad_(True)
        yd = m(xd, wd, noise=nz.to(dev()))
        np.testing.assert_allclose(yd.detach().cpu().numpy(), yo.detach().numpy(), **_tol(yo.detach().numpy()))
        gxd, gwd = torch.autograd.grad(yd, (xd, wd), go.to(dev()), create_graph=True)
        np.testing.assert_allclose(gxd.detach().cpu().numpy(), gxo.detach().numpy(), **_tol(gxo.detach().numpy(), 1e-4))
        np.testing.assert_allclose(gwd.detach().cpu().numpy(), gwo.detach().numpy(), **_tol(gwo.detach().numpy(), 1e-4))
        pen_d = gxd.pow(2).sum() + gwd.pow(2).sum()
        ggd, = torch.autograd.grad(pen_d, wd)
        np.testing.assert_allclose(ggd.cpu().numpy(), ggo.numpy(), **_tol(ggo.numpy(), 5e-4))


def test_modconv_random_shapes_vs_c_oracle():
    """Seeded sweep over batch / channel / size combinations of all three modes: every tile configuration (128-, 64-,
    32-channel tiles, tiny-layer packing, split-K, thin edge segments of the transposed conv) vs the C oracle."""
    from op import _native
    from oracle import c_oracle
    rng = np.random.default_rng(31)
    for n in range(24):
        mode = n % 3
        b = int(rng.integers(1, 5))
        cin = int(rng.choice([3, 8, 12, 20, 33, 64]))
        cout = int(rng.choice([5, 24, 40, 64, 100, 130]))
        h, w = int(rng.integers(3, 60)), int(rng.integers(3, 90))
        if mode == 0 and n % 2:
            h, w = int(rng.integers(40, 70)), int(rng.integers(50, 90))       # > 2048 positions: the large-layer tiles
        x = rng.standard_normal((b, cin, h, w)).astype(np.float32)
        wgt = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
        s = (1.0 + 0.5 * rng.standard_normal((b, cin))).astype(np.float32)
        demod = bool(n % 4)
        ref = c_oracle.modulated_conv2d(x, wgt, s, mode=mode, demodulate=demod)
        scale = 1.0 / np.sqrt(cin * 9)
        xd, wd, sd = (torch.from_numpy(t).to(dev()) for t in (x, wgt, s))
        wt = _native.modconv_weight_prep(wd, scale)
        dm = _native.modconv_demod(wd, sd, scale) if demod else None
        y = _native.modconv2d(xd, wt, sd, dm, mode)
        np.testing.assert_allclose(y.cpu().numpy(), ref, err_msg=f'mode {mode} b{b} {cin}->{cout} {h}x{w}', **_tol(ref))


# ---------------------------------------------------------------------------------------- index-range guard boundary
# Shapes just INSIDE the guards of fmgan_modconv2d_f32 (csrc/modconv_fwd.hip: 32-bit per-tile input offsets
# nb*cin*h*w < 2^31 elements; buffer-load staging only for tensors shorter than the parked voffset 0xFFFFFFF0 bytes)
# must compute correctly; shapes just outside return FMGAN_EOVERFLOW without launching (tests/test_abi_host.py).
# The tensors are 4-9 GB, so the check is the convolution's locality: output windows (all four corners, the last
# rows/columns, the middle) against the C oracle run on the matching input crop (tests/parity.py: window_check).


@pytest.mark.parametrize('cfg', [
    # (cin, cout, h, w, mode, what)
    (8, 8, 8192, 16383, 0, 'buffer-load staging, 0xFFF0_0000 bytes of input: just below the parked-voffset limit'),
    (8, 8, 8192, 16384, 0, 'exactly 2^32 bytes of input: guarded staging path'),
    (8, 8, 16384, 16383, 0, '2^31 - 2^17 input elements: just inside the 32-bit offset guard'),
    (8, 4, 8192, 16383, 1, 'transposed conv, input just below the parked-voffset limit, 8.6 GB output'),
], ids=['fastx_max', 'fastx_off', 'offset_guard_max', 'fastx_max_transposed'])
def test_guard_boundary_shapes_compute_correctly(cfg):
    from op import _native
    cin, cout, h, w, mode, _ = cfg
    gen = torch.Generator(device=dev()).manual_seed(1234)
    xd = torch.randn(1, cin, h, w, device=dev(), generator=gen)
    wgt = synth.tensor(f'guard/{cfg[:5]}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'guard/{cfg[:5]}/s', (1, cin), shift=1.0, scale=0.5)
    scale = 1.0 / np.sqrt(cin * 9)
    wd, sd = wgt.to(dev()), s.to(dev())
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    y = _native.modconv2d(xd, wt, sd, dm, mode)
    oh, ow = y.shape[2:]
    assert (oh, ow) == ((2 * h + 1, 2 * w + 1) if mode == 1 else (h, w))
    # windows reach the last output row and column; for the transposed conv (odd output sizes) origins are even
    wsz = 25 if mode == 1 else 24
    ey, ex = oh - wsz, ow - wsz
    mid_y, mid_x = (oh // 2) & ~1, (ow // 3) & ~1
    wins = [(0, 0), (0, ex), (ey, 0), (ey, ex), (mid_y, mid_x), (ey, mid_x), (mid_y, ex)]
    for (y0, x0) in wins:
        _window_check(xd, wgt, s, y, mode, y0, x0, wsz, wsz)
    assert torch.isfinite(y[:, :, ::997, ::991]).all()
    del y, xd
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------- nested dense-conv Functions
@pytest.mark.parametrize('cfg', [
    # (mode, b, cin, cout, h, w)
    (0, 2, 6, 10, 9, 7), (1, 2, 6, 10, 5, 6), (2, 2, 6, 10, 9, 11), (2, 1, 5, 7, 8, 10), (0, 1, 40, 24, 20, 20),
    (1, 3, 12, 33, 8, 8),
])
def test_dense_conv_family_differentiates_into_itself(cfg):
    """op.modconv.DenseConv / DenseConvDgrad / DenseConvWgrad (the create_graph=True path of ModulatedConv2d) against
    float64 autograd over torch's functional convs on the CPU: first, second and third derivatives, every mode (mode 2
    with an even-sized input, whose last row/column the stride-2 valid conv never reads)."""
    from op import modconv
    import torch.nn.functional as F
    mode, b, cin, cout, h, w = cfg
    u = synth.tensor(f'dcf/{cfg}/u', (b, cin, h, w))
    wt = synth.tensor(f'dcf/{cfg}/w', (cout, cin, 3, 3), scale=0.3)

    def ref_conv(uu, ww):
        if mode == 0:
            return F.conv2d(uu, ww, padding=1)
        if mode == 1:
            return F.conv_transpose2d(uu, ww.transpose(0, 1), stride=2)
        return F.conv2d(uu, ww, stride=2)

    def chain(conv, uu, ww, dt, device):
        y = conv(uu, ww)
        g1 = synth.tensor(f'dcf/{cfg}/g1', y.shape).to(device=device, dtype=dt)
        gu, gw = torch.autograd.grad(y, (uu, ww), g1, create_graph=True)
        l2 = gu.pow(2).mean() * gw.pow(2).mean()                                     # couples D_m and G_m
        hu, hw = torch.autograd.grad(l2, (uu, ww), create_graph=True)                # their derivatives: C, D, G again
        l3 = hu.pow(2).mean() + hw.pow(2).mean()
        tu, tw = torch.autograd.grad(l3, (uu, ww))                                   # third order
        return [t.detach().cpu().double().numpy() for t in (y, gu, gw, hu, hw, tu, tw)]

    ro = chain(ref_conv, u.double().requires_grad_(True), wt.double().requires_grad_(True), torch.float64, 'cpu')
    rd = chain(lambda a, c: modconv.DenseConv.apply(a, c, mode), u.to(dev()).requires_grad_(True),
               wt.to(dev()).requires_grad_(True), torch.float32, dev())
    for name, a, r, k in zip('y gu gw hu hw tu tw'.split(), rd, ro, (2e-5, 2e-5, 5e-5, 1e-4, 1e-4, 5e-4, 5e-4)):
        np.testing.assert_allclose(a, r, atol=k * max(1e-6, float(np.abs(r).max())), rtol=k * 10, err_msg=name)


def test_create_graph_path_runs_on_hip_kernels():
    """With a graph requested, ModulatedConv2d's backward must go through the DenseConv family (this repo's kernel),
    not through F.conv2d: count the MFMA-kernel launches the observer sees during backward + double backward."""
    import stylegan2
    m = load(stylegan2.StyledConv(6, 10, 3, 512, upsample=True), 'generator', 11, eval=False)
    x = synth.tensor('cgp/x', (2, 6, 5, 5)).to(dev()).requires_grad_(True)
    w = synth.tensor('cgp/w', (2, 512)).to(dev()).requires_grad_(True)
    y = m(x, w, noise=synth.tensor('cgp/n', (2, 1, 10, 10)).to(dev()))
    with launches.observed() as obs:
        gx, = torch.autograd.grad(y.sum(), x, create_graph=True)
        first = obs.count('modconv2d')
        gx.pow(2).sum().backward()
        second = obs.count('modconv2d') - first
    assert first >= 2, obs.names       # recomputed forward C + data gradient D on the MFMA kernel
    assert second >= 2, obs.names      # their derivatives, again on the MFMA kernel


@pytest.mark.parametrize('shape', [
    # (mode, b, cin, cout, h, w) with h, w the conv input's size: transposed (mode 1) and stride-2 (mode 2) weight gradients
    (1, 2, 64, 64, 16, 16), (1, 1, 128, 64, 32, 32), (1, 3, 100, 50, 17, 20), (1, 2, 512, 256, 64, 64),
    (2, 2, 64, 96, 35, 35), (2, 1, 70, 130, 40, 66), (2, 2, 128, 128, 129, 129)])
def test_strided_wgrad_kernel_vs_fp64(shape):
    """fmgan_modconv_wgrad_mode_f32 for the transposed and the stride-2 conv vs float64 autograd of the dense conv."""
    from op import _native
    import torch.nn.functional as F
    mode, b, cin, cout, h, w = shape
    x = synth.tensor(f'swg/{shape}/x', (b, cin, h, w)).to(dev())
    s = synth.tensor(f'swg/{shape}/s', (b, cin), shift=1.0, scale=0.5).to(dev())
    d = synth.tensor(f'swg/{shape}/d', (b, cout), shift=1.0, scale=0.3).to(dev())
    oh, ow = (2 * h + 1, 2 * w + 1) if mode == 1 else ((h - 3) // 2 + 1, (w - 3) // 2 + 1)
    go = synth.tensor(f'swg/{shape}/go', (b, cout, oh, ow)).to(dev())
    gw = _native.modconv_wgrad(go, d, x, s, 0.37, mode=mode)
    assert gw is not None
    wref = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, device=dev(), requires_grad=True)
    u64, g64 = (x * s[:, :, None, None]).double(), (go * d[:, :, None, None]).double()
    y = F.conv_transpose2d(u64, wref.transpose(0, 1), stride=2) if mode == 1 else F.conv2d(u64, wref, stride=2)
    ref, = torch.autograd.grad(y, wref, g64)
    ref = ref * 0.37
    torch.testing.assert_close(gw.double(), ref, atol=2e-5 * float(ref.abs().max()), rtol=2e-5)
    assert torch.equal(gw, _native.modconv_wgrad(go, d, x, s, 0.37, mode=mode))      # bit-reproducible


_LOOP_WORKER = r'''
import hashlib, json, os, sys
root = sys.argv[1]
for p in (root, os.path.join(root, '3d-fm-gan_amd')):
    sys.path.insert(0, p)
import torch
from op import _native
d = torch.device('cuda', 0)
out = {}
sel = {}
# (h, w, cin, cout, mode, batch): lean-loop shapes of every LDS-DMA tile (whole 4- and 8-channel chunks, whole channel tiles),
# a ragged-channel shape and a tiny one (general loop both times)
for (r, rw, cin, cout, mode, b) in [(64, 64, 128, 128, 0, 4), (32, 32, 64, 64, 0, 8), (32, 32, 32, 32, 0, 8), (32, 32, 128, 64, 1, 4),
                                    (64, 64, 64, 32, 1, 2), (33, 33, 40, 72, 0, 3), (17, 17, 24, 48, 1, 2), (8, 8, 64, 64, 0, 2),
                                    # the 256-position default tiles: plain C of the 128- and 64-channel classes, E
                                    (512, 64, 16, 128, 0, 4), (512, 64, 16, 64, 0, 4), (257, 36, 16, 32, 0, 8),
                                    # the transposed 64-channel DMA tile ((32, 32, 128, 64, 1, 4) above falls back to 'A':
                                    # its thin segments' patches put the LDS image over the limit)
                                    (33, 34, 32, 64, 1, 3)]:
    g = torch.Generator(device=d).manual_seed(r * 7 + mode)
    x = torch.randn(b, cin, r, rw, device=d, generator=g)
    w = torch.randn(cout, cin, 3, 3, device=d, generator=g)
    s = torch.randn(b, cin, device=d, generator=g) * 0.5 + 1
    wt = _native.modconv_weight_prep(w, 1.0 / (cin * 9) ** 0.5)
    dm = _native.modconv_demod(w, s, 1.0 / (cin * 9) ** 0.5)
    y = _native.modconv2d(x, wt, s, dm, mode)
    out[f'{r}x{rw}/{cin}/{cout}/{mode}/{b}'] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
    sel[f'{r}x{rw}/{cin}/{cout}/{mode}/{b}'] = [mode] + list(_native.modconv2d_select(b, cin, cout, r, rw, mode))
print('LIB ' + os.path.realpath(_native.LIB_PATH))
print('SELECT ' + json.dumps(sel))
print('DIGESTS ' + json.dumps(out))
'''


def test_lean_k_loop_equals_general_k_loop_bitwise(tmp_path):
    """csrc/modconv_fwd.hip, PIPE 1: the lean K loop (taken when every chunk is complete and DMA-servable) against the
    general loop: same DMA pieces, same MFMA order -> identical output bits on every tile family.  Only the experiments
    build of the library reads FMGAN_MC_DEBUG (=8 forces the general loop; read once, hence two processes), so the general
    loop runs on tools/exp/lib/libfmgan_hip_exp.so and the lean loop on the product library.  The worker also reports
    fmgan_modconv2d_select for every shape: both libraries must have run the same tiles, and the shapes must reach all eight
    LDS-DMA tiles of the product table (plain C / B of the 128- and 64-channel classes, plain E / B of the 32-channel class,
    transposed B and D) — each with a shape of whole chunks and whole channel tiles, the lean loop's."""
    import json
    import subprocess
    import sys
    script = tmp_path / 'loop_worker.py'
    script.write_text(_LOOP_WORKER)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = os.path.join(root, 'tools', 'exp', 'lib', 'libfmgan_hip_exp.so')
    if not os.path.exists(exp):
        subprocess.check_call(['make', '-C', os.path.join(root, '3d-fm-gan_amd', 'csrc'), '-j16', 'experiments'])
    res, libs, sels = [], [], []
    for dbg, lib in (('0', None), ('8', exp)):
        env = dict(os.environ, FMGAN_MC_DEBUG=dbg)
        env.pop('FMGAN_LIB', None)
        if lib:
            env['FMGAN_LIB'] = lib
        pr = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in pr.stdout.splitlines() if ln.startswith('DIGESTS ')]
        used = [ln for ln in pr.stdout.splitlines() if ln.startswith('LIB ')]
        picked = [ln for ln in pr.stdout.splitlines() if ln.startswith('SELECT ')]
        assert pr.returncode == 0 and line and used and picked, pr.stdout[-1000:] + pr.stderr[-3000:]
        res.append(json.loads(line[0][8:]))
        libs.append(used[0][4:])
        sels.append(json.loads(picked[0][7:]))
    assert libs[0] != libs[1] and libs[1] == os.path.realpath(exp), libs
    # both libraries ran the same tile on every shape, and the shapes reach all eight LDS-DMA tiles of the product table
    assert sels[0] == sels[1], (sels[0], sels[1])
    reached = {(m, cfg, v) for (m, cfg, v, _bm, _bn, _ks) in sels[0].values()}
    dma = {(0, 0, 'C'), (0, 0, 'B'), (0, 1, 'C'), (0, 1, 'B'), (0, 2, 'E'), (0, 2, 'B'), (1, 1, 'B'), (1, 2, 'D')}
    from op import _native
    assert dma == {(m, cfg, v) for (m, cfg, v, _bm, _bn, _rgb) in _native.modconv2d_tiles() if v != 'A'}
    assert dma <= reached, sorted(dma - reached)
    assert res[0] == res[1]
    assert len(res[0]) == 12 and len(sels[0]) == 12
