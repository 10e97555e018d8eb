"""GPU tests of the reduced-precision modulated conv (fmgan_modconv2d_bf16, BASELINE config 5's bf16 leg).

Not a parity row: the reference has no bf16 path.  The kernel is held to its own definition — bf16-rounded operands,
exact products, fp32 accumulation — through oracle/torch_oracle.py::modconv_bf16_reference (float64 convolution of the
rounded operands): 2e-5 of max|out|, i.e. fp32 summation error only; and to the bf16-sized distance from the fp32 kernel
SURVEY §8c states for this configuration (5e-2 on [-1,1] images end to end; per layer a few 1e-3 of max|out|)."""
import numpy as np
import pytest
import torch

import synth
from gpumem import dev
from launches import observed
from modconv_bf16_cases import inputs as _inputs
from nets import load
from parity import no_farther_than_reference

pytestmark = pytest.mark.gpu


CASES = [
    # (b, cin, cout, h, w, mode): every tile configuration (cout 32 / >= 64), ragged grids, several chunks
    (2, 32, 32, 64, 64, 0), (1, 16, 32, 40, 33, 0), (2, 64, 64, 32, 32, 0), (1, 48, 96, 37, 70, 0), (3, 128, 160, 36, 32, 0),
    (2, 32, 32, 64, 64, 1), (1, 16, 32, 9, 33, 1), (2, 64, 64, 32, 32, 1), (1, 48, 96, 21, 45, 1),
    (2, 32, 32, 129, 129, 2), (1, 16, 64, 75, 67, 2), (1, 64, 32, 67, 131, 2), (2, 32, 96, 11, 65, 2),
]


@pytest.mark.parametrize('cfg', CASES)
@pytest.mark.parametrize('demod', [True, False])
def test_bf16_kernel_matches_its_definition(cfg, demod):
    from op import _native
    from oracle import torch_oracle as T
    b, cin, cout, h, w, mode = cfg
    x, wgt, s, scale = _inputs(cfg)
    assert _native.lib().fmgan_modconv2d_bf16_supported(b, cin, cout, h, w, mode) == 1
    xd, wd, sd = x.to(dev()), wgt.to(dev()), s.to(dev())
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale) if demod else None
    y = _native.modconv2d(xd, wt, sd, dm, mode, precision='bf16')
    ref = T.modconv_bf16_reference(x, wgt, s, None if dm is None else dm.cpu(), mode, scale).numpy()
    assert y.shape == ref.shape
    np.testing.assert_allclose(y.cpu().numpy(), ref, atol=2e-5 * float(np.abs(ref).max()), rtol=0)
    # bf16-sized distance from the fp32 kernel (operand rounding 2^-9 each, averaged over cin*9 products)
    y32 = _native.modconv2d(xd, wt, sd, dm, mode, precision='f32')
    err = float((y - y32).abs().max() / y32.abs().max())
    assert 1e-5 < err < 1e-2, err
    with _native.modconv_precision('bf16'):
        assert torch.equal(_native.modconv2d(xd, wt, sd, dm, mode), y)      # ambient switch, bit-reproducible
    assert torch.equal(_native.modconv2d(xd, wt, sd, dm, mode), y32)        # and it is off again outside


@pytest.mark.parametrize('precision', ['bf16', 'bf16x3'])
@pytest.mark.parametrize('shape', [(2, 32, 64, 40, 64), (1, 16, 96, 9, 33)])
def test_bf16_fused_epilogue_and_strided_output(precision, shape):
    """Plain conv with noise + bias + lrelu in the epilogue, and the transposed conv writing the aligned-row intermediate:
    same values as the separate steps on the result of the same precision.  The second shape has a ragged last channel
    tile on the bf16 kernel's 64-channel tile in mode 0 (the predicated stores, with the activation) and a 10 x 34 quad
    grid in mode 1 (tiles stored through the buffer resource and ragged ones in both directions, in one launch)."""
    from op import _native
    cfg = shape + (0,)
    b, cin, cout, h, w, _ = cfg
    supported = getattr(_native.lib(), f'fmgan_modconv2d_{precision}_supported')
    assert supported(b, cin, cout, h, w, 0) == 1 and supported(b, cin, cout, h, w, 1) == 1
    x, wgt, s, scale = _inputs(cfg)
    d = dev()
    xd, wd, sd = x.to(d), wgt.to(d), s.to(d)
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    nz = synth.tensor('bf/ep/n', (b, 1, h, w)).to(d)
    nw = torch.tensor([0.41], device=d)
    bias = synth.tensor('bf/ep/b', (cout,)).to(d)
    plain = _native.modconv2d(xd, wt, sd, dm, 0, precision=precision)
    fused = _native.modconv2d(xd, wt, sd, dm, 0, noise=nz, noise_weight=nw, bias=bias, fuse_act=True, precision=precision)
    assert torch.equal(fused, _native.noise_bias_act(plain, nz, nw, bias, 0.2, 2 ** 0.5))
    up = _native.modconv2d(xd, wt, sd, dm, 1, precision=precision)
    oh, ow = 2 * h + 1, 2 * w + 1
    buf, p0, ps, rs = _native.aligned_rows_buffer(b, cout, oh, ow, 1, d)
    buf.fill_(float('nan'))
    _native.modconv2d(xd, wt, sd, dm, 1, strided_out=(p0, ps, rs), precision=precision)
    assert torch.equal(buf[:, :, 1:1 + ow].reshape(b, cout, oh, ow), up)
    assert torch.isnan(buf[:, :, 0]).all() and torch.isnan(buf[:, :, 1 + ow:]).all()


def test_bf16_unsupported_shapes_keep_the_fp32_kernel():
    from op import _native
    L = _native.lib()
    for cfg in ((2, 12, 32, 64, 64, 0), (2, 32, 48, 64, 64, 0), (2, 32, 32, 16, 16, 0), (2, 512, 512, 4, 4, 1), (1, 32, 32, 40, 40, 2)):
        assert L.fmgan_modconv2d_bf16_supported(*cfg) == 0, cfg
    cfg = (2, 12, 32, 64, 64, 0)
    x, wgt, s, scale = _inputs(cfg)
    xd, wd, sd = x.to(dev()), wgt.to(dev()), s.to(dev())
    wt = _native.modconv_weight_prep(wd, scale)
    with _native.modconv_precision('bf16'):
        y = _native.modconv2d(xd, wt, sd, None, 0)
    assert torch.equal(y, _native.modconv2d(xd, wt, sd, None, 0))


def test_bf16_generator_forward_within_stated_tolerance():
    """Generator(256) forward with every served layer on the bf16 contraction vs the fp32 path: SURVEY §8c's stated
    tolerance for the bf16 configuration is 5e-2 on [-1,1]-scaled images; the synthetic weights here give images of
    max ~8, so the bound is taken relative to max|image|."""
    import stylegan2
    from op import _native
    G = load(stylegan2.Generator(256, 512, 2), 'generator', 4)
    lat = synth.tensor('bf/g/lat', (2, G.n_latent, 512)).to(dev())
    tsr = synth.tensor('bf/g/tsr', (2, 512, 4, 4)).to(dev())
    kw = dict(latent_styles=[lat], input_is_latent=True, use_external_input_tensor=True, external_input_tensor=tsr,
              randomize_noise=False)
    with torch.no_grad():
        ref = G(None, **kw)
        with _native.modconv_precision('bf16'):
            img = G(None, **kw)
    err = float((img - ref).abs().max() / ref.abs().max())
    assert 1e-5 < err < 5e-2, err
    # training graph (forward + data gradients on the bf16 kernel, weight gradients fp32): finite, close to fp32
    G.requires_grad_(True)
    tsr_g = tsr.clone().requires_grad_(True)
    kw['external_input_tensor'] = tsr_g
    g32, = torch.autograd.grad(G(None, **kw).abs().mean(), tsr_g)
    with _native.modconv_precision('bf16'):
        loss = G(None, **kw).abs().mean()
        with observed() as rec:
            g16, = torch.autograd.grad(loss, tsr_g)
    assert rec.count('modconv2d_bf16') >= 1, rec.names       # the data gradients ran on the bf16 kernel
    assert torch.isfinite(g16).all()
    assert float((g16 - g32).abs().max() / g32.abs().max()) < 0.1


def test_inference_and_training_under_autocast_are_safe():
    """torch.autocast(bfloat16) around the whole path (the bf16 leg): the style MLP then produces bf16 vectors and the
    library convs bf16 activations.  The fused inference forward and every autograd Function must see fp32 (they hand raw
    pointers to the library; round 3's first bf16 run faulted the GPU on a bf16 style vector): same image as without
    autocast up to the bf16 rounding of the style MLP, finite gradients."""
    import stylegan2
    from op import _native
    G = load(stylegan2.Generator(64, 512, 2), 'generator', 4)
    lat = synth.tensor('ac/lat', (2, G.n_latent, 512)).to(dev())
    tsr = synth.tensor('ac/tsr', (2, 512, 4, 4)).to(dev())
    kw = dict(latent_styles=[lat], input_is_latent=True, use_external_input_tensor=True, randomize_noise=False)
    with torch.no_grad():
        ref = G(None, external_input_tensor=tsr, **kw)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            a = G(None, external_input_tensor=tsr, **kw)
            b = G(None, external_input_tensor=tsr.bfloat16(), **kw)       # what an autocast encoder hands over
            with _native.modconv_precision('bf16'):
                c = G(None, external_input_tensor=tsr, **kw)
    for img in (a, b, c):
        assert img.dtype == torch.float32 and torch.isfinite(img).all()
        assert float((img - ref).abs().max() / ref.abs().max()) < 5e-2
    G.requires_grad_(True)
    t = tsr.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16), _native.modconv_precision('bf16'):
        img = G(None, external_input_tensor=t, **kw)
        (img.float().abs().mean()).backward()
    assert torch.isfinite(t.grad).all() and all(torch.isfinite(p.grad).all() for p in G.parameters() if p.grad is not None)


# ------------------------------------------------------------------------------------------------ bf16x3: fp32 by splitting
X3_CASES = [(2, 32, 32, 64, 64, 0), (1, 16, 32, 40, 33, 0), (2, 64, 64, 32, 32, 0), (1, 48, 96, 37, 70, 0), (3, 128, 160, 36, 32, 0),
            (1, 512, 512, 64, 64, 0), (2, 32, 32, 64, 64, 1), (1, 16, 32, 9, 33, 1), (2, 64, 64, 32, 32, 1), (1, 48, 96, 21, 45, 1),
            (1, 512, 256, 64, 64, 1)]


@pytest.mark.parametrize('cfg', X3_CASES)
@pytest.mark.parametrize('demod', [True, False])
def test_bf16x3_kernel_has_fp32_accuracy(cfg, demod):
    """fmgan_modconv2d_bf16x3 (fp32 operands split into three bf16 pieces, six bf16 MFMAs per product) against a float64
    convolution of the UNROUNDED operands: it must be as accurate as the fp32 MFMA kernel — its error vs float64 at most
    2x the fp32 kernel's + 2e-6 of max|out| — and within the fp32 kernel's oracle tolerance (2e-5) of it."""
    from op import _native
    b, cin, cout, h, w, mode = cfg
    x, wgt, s, scale = _inputs(cfg)
    assert _native.lib().fmgan_modconv2d_bf16x3_supported(b, cin, cout, h, w, mode) == 1
    xd, wd, sd = x.to(dev()), wgt.to(dev()), s.to(dev())
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale) if demod else None
    y3 = _native.modconv2d(xd, wt, sd, dm, mode, precision='bf16x3')
    y32 = _native.modconv2d(xd, wt, sd, dm, mode, precision='f32')
    u = (x.float() * s.float()[:, :, None, None]).double()
    wq = (wgt.float() * torch.tensor(scale, dtype=torch.float32)).double()
    ref = torch.nn.functional.conv2d(u, wq, padding=1) if mode == 0 else torch.nn.functional.conv_transpose2d(u, wq.transpose(0, 1), stride=2)
    if dm is not None:
        ref = ref * dm.cpu().double()[:, :, None, None]
    mx = float(ref.abs().max())
    e3 = float((y3.cpu().double() - ref).abs().max()) / mx
    e32 = float((y32.cpu().double() - ref).abs().max()) / mx
    assert e3 <= 2 * e32 + 2e-6, (e3, e32)
    assert float((y3 - y32).abs().max()) / mx <= 2e-5
    assert torch.equal(_native.modconv2d(xd, wt, sd, dm, mode, precision='bf16x3'), y3)      # bit-reproducible


def test_bf16x3_generator_meets_the_fp32_path_gates(golden):
    """Generator(256) and Generator(1024) full width with every served layer on the split-operand contraction: the fp32
    path's own gates — 1e-4 vs the reference's fp32 image (BASELINE §4) and 'no farther from the float64 image than
    4 x the reference's fp32 error + 2e-6' (tests/test_hip_models.py)."""
    import cases
    import stylegan2
    from op import _native
    g32, g64 = golden('generator'), golden('fp64')
    for c in cases.GENERATOR_CASES:
        if c['name'] not in ('g256_full', 'g1024_full'):
            continue
        G = load(stylegan2.Generator(c['size'], 512, c['n_mlp']), 'generator', 4)
        lat = synth.tensor(c['name'] + '/latent', (c['b'], G.n_latent, 512)).to(dev())
        tsr = synth.tensor(c['name'] + '/tsr', (c['b'], 512, 4, 4)).to(dev())
        with torch.no_grad(), _native.modconv_precision('bf16x3'):
            img = G(None, latent_styles=[lat], input_is_latent=True, use_external_input_tensor=True,
                    external_input_tensor=tsr, randomize_noise=False)
        a = img.cpu().numpy()[..., ::c['stride'], ::c['stride']]
        r32, r64 = g32[c['name'] + '/sub'], g64[c['name'] + '/sub']
        mx = float(np.abs(r64).max())
        np.testing.assert_allclose(a, r32, atol=1e-4 * mx, rtol=1e-4)
        no_farther_than_reference(a, r32, r64)
        del G
