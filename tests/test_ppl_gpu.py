"""GPU tests of the perceptual path length: the input-stage kernel (csrc/ppl_input.hip) bit for bit against its stated
formula, against F.interpolate, and the Generator cases of tests/ppl_cases.py through Evaluation.ppl.PPL_Distances against
the reference's values (tests/golden/ppl.npz), with the fused and the composite input stage."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import launches
import nets
import ppl_cases as pc
import synth
from gpumem import dev, guarded, guards_intact
from nets import PinNoise, load, scaling

pytestmark = pytest.mark.gpu


def expected(img, shift, scale, window, f):
    """The header's formula in fp32 torch ops on strided slices of the window: v, then u = v - shift in fp32, then the
    float64 quotient rounded to fp32 (= the correctly rounded fp32 quotient, however torch divides).  [2P, 3, oh, ow]."""
    y0, x0, hc, wc = window
    win = img[:, :, y0:y0 + hc, x0:x0 + wc]
    if f == 1:
        v = win
    else:
        o = f // 2 - 1
        a, b = win[:, :, o::f, o::f], win[:, :, o::f, o + 1::f]
        c, d = win[:, :, o + 1::f, o::f], win[:, :, o + 1::f, o + 1::f]
        v = 0.5 * (0.5 * a + 0.5 * b) + 0.5 * (0.5 * c + 0.5 * d)
    u = v - shift.view(1, 3, 1, 1)
    assert u.dtype == torch.float32
    return (u.double() / scale.view(1, 3, 1, 1).double()).float()


KERNEL_CASES = [
    # shape, f, window (None: the whole image)
    ((2, 3, 5, 7), 1, None),
    ((6, 3, 12, 20), 2, None),                       # three pairs
    ((2, 3, 16, 24), 4, None),
    ((2, 3, 16, 24), 4, (4, 3, 8, 20)),              # odd x0, a tail unit
    ((2, 3, 32, 32), 1, (12, 8, 16, 16)),            # the crop's geometry
    ((4, 3, 1024, 1024), 4, None),                   # production
    ((2, 3, 1024, 1024), 2, (384, 256, 512, 512)),   # production, cropped
]


@pytest.mark.parametrize('shape,f,window', KERNEL_CASES,
                         ids=['x'.join(map(str, s)) + f'-f{f}' + ('-window' if w else '') for s, f, w in KERNEL_CASES])
def test_kernel_against_the_formula_bit_for_bit(shape, f, window):
    """Pixels outside the window are NaN and the outputs are pre-filled with NaN between guard words: every output element
    is written, finite and equal to the formula's bits; no guard word changes.  The binding gives the same tensors."""
    from op import _native
    L = _native.lib()
    n, _, h, w = shape
    window = window or (0, 0, h, w)
    y0, x0, hc, wc = window
    values = synth.tensor('ppl/kernel/' + 'x'.join(map(str, shape)), shape, dist='uniform').to(dev())
    img = torch.full(shape, float('nan'), dtype=torch.float32, device=dev())
    img[:, :, y0:y0 + hc, x0:x0 + wc] = values[:, :, y0:y0 + hc, x0:x0 + wc]
    sl = scaling()
    shift, scale = sl.shift.reshape(3), sl.scale.reshape(3)
    oh, ow = hc // f, wc // f
    kernel = L.fmgan_lpips_pair_input_select(n // 2, h, w, y0, x0, hc, wc, f)
    assert kernel == (f if ow % 4 == 0 else 8 + f)
    (buf0, out0), (buf1, out1) = guarded((n // 2, oh, ow, 3)), guarded((n // 2, oh, ow, 3))
    st = L.fmgan_lpips_pair_input_f32(_native.fp(img), _native.fp(shift), _native.fp(scale), out0.data_ptr(),
                                      out1.data_ptr(), n // 2, h, w, y0, x0, hc, wc, f,
                                      torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    want = expected(img, shift, scale, window, f)
    assert tuple(want.shape) == (n, 3, oh, ow) and bool(torch.isfinite(want).all())
    for buf, out, ref in ((buf0, out0, want[::2]), (buf1, out1, want[1::2])):
        assert guards_intact(buf)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out.permute(0, 3, 1, 2), ref)
    got = _native.lpips_pair_input(img, sl.shift, sl.scale, window, f)
    for t, out in zip(got, (out0, out1)):
        assert tuple(t.shape) == (n // 2, 3, oh, ow) and t.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(t, out.permute(0, 3, 1, 2))


@pytest.mark.parametrize('size,f', [(512, 2), (1024, 4)])
def test_kernel_against_interpolate(size, f):
    """With shift 0 and scale 1 the kernel's 256^2 images against F.interpolate on the GPU, within 2^-22 * max|x| (three
    roundings per form at magnitudes <= max|x|, two of them halved, two forms: tests/test_ppl.py); whether they are
    bit-equal is printed."""
    from op import ppl_input as PI
    x = synth.tensor(f'ppl/interp/{size}', (2, 3, size, size), dist='uniform').to(dev())
    sl = scaling()
    sl.shift.zero_()
    sl.scale.fill_(1.0)
    assert PI.pair_input_serves(x) and PI.pair_input_plan(tuple(x.shape), False) == ((0, 0, size, size), f)
    got = PI.pair_input(x, sl)
    want = F.interpolate(x, size=(256, 256), mode='bilinear', align_corners=False)
    gate = 2.0 ** -22 * float(x.abs().max())
    for g, w in zip(got, (want[::2], want[1::2])):
        err = float((g - w).abs().max())
        print(f'{size} f={f}: max|kernel - F.interpolate| {err:.3e} gate {gate:.3e} bit-equal {torch.equal(g, w)}')
        assert tuple(g.shape) == (1, 3, 256, 256) and err <= gate
    comp = PI.pair_input(x, sl, fuse=False)
    for g, c in zip(got, comp):
        assert c.is_contiguous(memory_format=torch.channels_last) and float((g - c).abs().max()) <= gate


# ------------------------------------------------------------------------------------------------ Generator cases
_generators = {}


def _generator(size):
    import stylegan2
    if size not in _generators:
        _generators[size] = load(stylegan2.Generator(size, 512, 8), 'generator', 4)
    return _generators[size]


@pytest.fixture(scope='module')
def percept():
    return nets.percept(dev())


@pytest.mark.parametrize('fuse', [True, False], ids=['fused', 'composite'])
@pytest.mark.parametrize('name', ['g64', 'g512', 'g512_crop'])
def test_generator_cases_golden(name, fuse, golden, percept):
    """Per pair against the reference's float64 run: |d - dist64| <= 4 * max over the case's pairs |dist32 - dist64| (the
    project's standing rule for an fp32 path against the reference's own fp32 error).  Each figure is printed before it is
    asserted.  The fused form's shapes are served (asserted through the library's select)."""
    from Evaluation import ppl as P
    from op import _native, ppl_input as PI
    c = pc.BY_NAME[name]
    g = golden('ppl')
    gen = PinNoise(_generator(c['size']))
    plan = PI.pair_input_plan((2 * c['batch'], 3, c['size'], c['size']), c['crop'])
    assert plan is not None
    (y0, x0, hc, wc), f = plan
    assert f == {'g64': 1, 'g512': 2, 'g512_crop': 1}[name]
    assert _native.lib().fmgan_lpips_pair_input_select(c['batch'], c['size'], c['size'], y0, x0, hc, wc, f) == f
    with launches.observed() as rec:
        d = P.PPL_Distances(gen, percept, c['n_sample'], c['batch'], c['eps'], c['latent_dim'], dev(),
                            sampler=pc.sampler(c), crop=c['crop'], fuse=fuse)
    assert rec.count('lpips_pair_input') == (c['n_sample'] // c['batch'] if fuse else 0)
    d32, d64 = g[name + '/dist'], g[name + '/dist64']
    assert tuple(d.shape) == d64.shape and d.dtype == torch.float32
    d = d.double().cpu().numpy()
    gate = 4 * np.abs(d32 - d64).max()
    err = np.abs(d - d64)
    for i in range(len(d)):
        print(f'{name} {"fused" if fuse else "composite"} pair {i}: d {d[i]:.9e} dist64 {d64[i]:.9e} |d - dist64| '
              f'{err[i]:.3e} reference |dist32 - dist64| {abs(d32[i] - d64[i]):.3e} gate {gate:.3e}')
    assert np.all(err <= gate), (err.max(), gate)


def test_generator_1024_one_batch(percept):
    """One batch of 2 pairs on Generator(1024), no crop: the f = 4 kernel serves the images; finite, positive distances."""
    from Evaluation import ppl as P
    from op import ppl_input as PI
    c = dict(name='g1024', batch=2, latent_dim=512)
    gen = PinNoise(_generator(1024))
    served = []
    call = gen._call[0]

    def checking(**kw):
        image = call(**kw)
        served.append((tuple(image.shape), PI.pair_input_serves(image)))
        return image
    gen._call[0] = checking
    d = P.PPL_Distances(gen, percept, 2, 2, 1e-2, 512, dev(), sampler=pc.sampler(c))
    assert served == [((4, 3, 1024, 1024), True)]
    assert tuple(d.shape) == (2,) and bool(torch.isfinite(d).all()) and bool((d > 0).all())
    print('g1024 distances', d.tolist())
