"""GPU tests of the FID's kernels and paths: the fp64-MFMA update and the finish kernel of csrc/fid_stats.hip through the
raw entry points, Feature_Statistics fused against composite, the Inception input stage of csrc/inception_input.hip,
Sample_Statistics on the Generator against the reference's FID, and the folded InceptionV3 forward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_cases as fc
import synth
from gpumem import GUARD, SENTINEL, dev, guarded, guards_intact
from launches import observed
from nets import lib, load

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -2


def guarded64(shape, fill):
    """(buf, view): float64 `view` of `shape` holding a copy of `fill`, between GUARD sentinels."""
    fill = torch.as_tensor(fill, dtype=torch.float64)
    n = fill.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev())
    buf[GUARD:GUARD + n] = fill.reshape(-1).to(dev())
    return buf, buf[GUARD:GUARD + n].view(shape)


def _stream():
    return torch.cuda.current_stream(dev()).cuda_stream


def _feat(tag, b, d):
    """relu-like fp32 features with a non-zero mean, full mantissas."""
    return torch.relu(synth.tensor(f'fid_gpu/{tag}/{b}x{d}', (b, d)) + 0.7)


# ------------------------------------------------------------------------------------------------ update kernel
def _exact_moments(feat, shift):
    """(sum_b y [d], sum_b y_i y_j [d, d], sum_b |y| [d], sum_b |y_i y_j| [d, d]) with y = float64(feat) - shift formed as
    the kernel forms it (one float64 subtraction), as longdouble (x87 extended, 64-bit mantissa).  The column sums are
    added in extended precision.  The second moments come from float64 matrix products made exact by splitting
    y = h + l on the grid 2^-17: |h| < 2^3, so h_i h_j is a multiple of 2^-34 below 2^6 and a sum of b <= 2^13 of them is
    exact in float64 in any order; l = y - h is exact with |l| <= 2^-18, so the three remaining products are 2^-17 of
    the whole and their float64 rounding is 2^-17 of the bound checked against the total."""
    y = feat.double().numpy() - shift
    assert float(np.abs(y).max()) < 8 and y.shape[0] <= 1 << 13
    h = np.round(y * 2.0 ** 17) / 2.0 ** 17
    low = y - h
    assert np.array_equal(h + low, y)
    rest = h.T @ low + low.T @ h + low.T @ low
    ay = np.abs(y)
    return y.astype(np.longdouble).sum(0), (h.T @ h).astype(np.longdouble) + rest, ay.sum(0), ay.T @ ay


UPDATE_SHAPES = [(1, 16), (3, 16), (5, 48), (7, 80), (9, 2048), (100, 2048)]


@pytest.mark.parametrize('b,d', UPDATE_SHAPES, ids=[f'{b}x{d}' for b, d in UPDATE_SHAPES])
def test_update_kernel(b, d):
    """fmgan_fid_stats_update_f32 into pre-filled accumulators between guards, twice (the second update accumulates onto
    the first's result).  Against the exact moments: |outer - (pre + P)| <= gamma_b * sum_b |y_i y_j| + u * |outer| and
    the same form for sum: b roundings for the b products in any order (the issue's bound), and one more for the in-place
    addition to the pre-filled value, which is a correctly rounded float64 addition whatever the kernel does.  Elements
    below the diagonal and the guards keep their bits."""
    L = lib()
    assert L.fmgan_fid_stats_select(b, d) == 1
    shift = synth.tensor(f'fid_gpu/shift/{d}', (d,), dtype=torch.float64, scale=0.3, shift=0.6)
    pre_sum = synth.tensor(f'fid_gpu/pre_sum/{d}', (d,), dtype=torch.float64, scale=3.0)
    pre_outer = synth.tensor(f'fid_gpu/pre_outer/{d}', (d, d), dtype=torch.float64, scale=3.0)
    bs, sum_ = guarded64((d,), pre_sum)
    bo, outer = guarded64((d, d), pre_outer)
    sh = shift.to(dev())
    low = np.tril_indices(d, -1)
    upper = np.triu(np.ones((d, d), dtype=bool))
    g = fc.gamma(b)
    state_sum, state_outer = pre_sum.numpy().copy(), pre_outer.numpy().copy()
    for step in range(2):
        feat = _feat(f'update{step}', b, d)
        fd = feat.to(dev())
        assert L.fmgan_fid_stats_update_f32(fd.data_ptr(), sh.data_ptr(), sum_.data_ptr(), outer.data_ptr(), b, d,
                                            _stream()) == 0
        got_sum, got_outer = sum_.cpu().numpy(), outer.cpu().numpy()
        s, p, abs_s, abs_p = _exact_moments(feat, shift.numpy())
        err_sum = np.abs(got_sum - (state_sum.astype(np.longdouble) + s)).astype(np.float64)
        err_outer = np.abs(got_outer - (state_outer.astype(np.longdouble) + p)).astype(np.float64)
        bound_sum = g * abs_s + fc.U * np.abs(got_sum)
        bound_outer = g * abs_p + fc.U * np.abs(got_outer)
        print(f'{b}x{d} update {step}: max err/bound sum {float((err_sum / bound_sum).max()):.3f} outer '
              f'{float((err_outer / bound_outer)[upper].max()):.3f}')
        assert (err_sum <= bound_sum).all()
        assert (err_outer <= bound_outer)[upper].all()
        assert np.array_equal(got_outer[low], pre_outer.numpy()[low])
        assert bool((bs[:GUARD] == SENTINEL).all()) and bool((bs[-GUARD:] == SENTINEL).all())
        assert bool((bo[:GUARD] == SENTINEL).all()) and bool((bo[-GUARD:] == SENTINEL).all())
        state_sum, state_outer = got_sum, got_outer


def test_update_declines_unserved_width_and_writes_nothing():
    L = lib()
    assert L.fmgan_fid_stats_select(4, 24) == EUNSUP
    feat = _feat('declined', 4, 24).to(dev())
    sh = torch.zeros(24, dtype=torch.float64, device=dev())
    bs, sum_ = guarded64((24,), torch.full((24,), 2.5))
    bo, outer = guarded64((24, 24), torch.full((24, 24), 2.5))
    assert L.fmgan_fid_stats_update_f32(feat.data_ptr(), sh.data_ptr(), sum_.data_ptr(), outer.data_ptr(), 4, 24,
                                        _stream()) == EUNSUP
    torch.cuda.synchronize()
    assert bool((sum_ == 2.5).all()) and bool((outer == 2.5).all())
    assert bool((bs[:GUARD] == SENTINEL).all()) and bool((bo[-GUARD:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ finish, the class
def _check_against_numpy(mean, cov, feat, shift):
    f64 = feat.double().numpy()
    mean_bound, cov_bound = fc.moment_bounds(f64, shift)
    want_mean, want_cov = np.mean(f64, 0), np.cov(f64, rowvar=False)
    print('max |mean diff| / bound', float((np.abs(mean - want_mean) / mean_bound).max()),
          'max |cov diff| / bound', float((np.abs(cov - want_cov) / cov_bound).max()))
    assert (np.abs(mean - want_mean) <= mean_bound).all()
    assert (np.abs(cov - want_cov) <= cov_bound).all()
    return mean_bound, cov_bound


@pytest.mark.parametrize('d', [80, 2048])
def test_finish_kernel(d):
    """fmgan_fid_stats_finish_f64 on the moments of three updates: cov is bit-symmetric, mean / cov are np.mean / np.cov of
    the same features within fid_cases.moment_bounds; n = 1 is FMGAN_EINVAL."""
    L = lib()
    feat = _feat('finish', 111, d)
    shift = feat[:37].double().mean(0)
    sh = shift.to(dev())
    sum_ = torch.zeros(d, dtype=torch.float64, device=dev())
    outer = torch.full((d, d), float('nan'), dtype=torch.float64, device=dev()).tril_(-1)   # NaN below the diagonal only:
    assert bool(torch.isnan(outer[1, 0])) and float(outer[0, 1]) == 0.0                    # never read, never written
    for i in range(0, 111, 37):
        part = feat[i:i + 37].to(dev())
        assert L.fmgan_fid_stats_update_f32(part.data_ptr(), sh.data_ptr(), sum_.data_ptr(), outer.data_ptr(), 37, d,
                                            _stream()) == 0
    bm, mean = guarded64((d,), torch.zeros(d))
    bc, cov = guarded64((d, d), torch.zeros(d, d))
    args = (sum_.data_ptr(), outer.data_ptr(), sh.data_ptr())
    assert L.fmgan_fid_stats_finish_f64(*args, 1, mean.data_ptr(), cov.data_ptr(), d, _stream()) == EINVAL
    assert L.fmgan_fid_stats_finish_f64(*args, 111, mean.data_ptr(), cov.data_ptr(), d, _stream()) == 0
    assert torch.equal(cov, cov.T) and bool(torch.isfinite(cov).all())
    _check_against_numpy(mean.cpu().numpy(), cov.cpu().numpy(), feat, shift.numpy())
    for buf in (bm, bc):
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize('d', [64, 2048, 52], ids=['d64', 'd2048', 'd52_composite'])
def test_feature_statistics_fused_against_composite(d):
    """The same batches (37, 37, 26) through the kernel path and the float64 torch composite: each within
    fid_cases.moment_bounds of numpy, and within the same bounds of each other; one launch bracket per update where the
    kernel serves (d % 16 == 0), none elsewhere."""
    from op.fid_stats import Feature_Statistics
    feat = _feat('class', 100, d)
    states = {}
    for fuse in (True, False):
        st = Feature_Statistics(d, dev(), fuse=fuse)
        with observed() as rec:
            for i in range(0, 100, 37):
                st.update(feat[i:i + 37].to(dev()))
        updates = [info for info in rec.infos('fid_stats') if info[2] == 0]
        assert len(updates) == (3 if fuse and d % 16 == 0 else 0), rec.seen
        mean, cov = st.finish()
        assert mean.dtype == torch.float64 and cov.is_cuda and torch.equal(cov, cov.T) and st.count == 100
        states[fuse] = (mean.cpu().numpy(), cov.cpu().numpy(), st.shift.cpu().numpy())
    mean_bound, cov_bound = _check_against_numpy(*states[True][:2], feat, states[True][2])
    _check_against_numpy(*states[False][:2], feat, states[False][2])
    assert (np.abs(states[True][0] - states[False][0]) <= mean_bound).all()
    assert (np.abs(states[True][1] - states[False][1]) <= cov_bound).all()


# ------------------------------------------------------------------------------------------------ input stage
def _taps(s, device):
    """(i0, i1, l0, l1) per output index by the header's rule: src = fmaf(scale, d + 0.5, -0.5) with ONE rounding (taken
    here as the fp32 rounding of the float64 expression, which is exact before it), clamped at 0."""
    scale = torch.tensor(float(s), dtype=torch.float32, device=device) / 299
    d = torch.arange(299, dtype=torch.float32, device=device) + 0.5
    src = (scale.double() * d.double() - 0.5).float().clamp_min(0)
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < s - 1).to(torch.int64)
    l1 = src - i0.float()
    return i0, i1, 1 - l1, l1


def _formula(x, normalize):
    """The header's formula in fp32 torch ops (each a single rounded operation)."""
    s = x.shape[-1]
    if s == 299:
        v = x
    else:
        i0, i1, l0, l1 = _taps(s, x.device)
        r0, r1 = x[:, :, i0], x[:, :, i1]
        a, b, c, d = r0[..., i0], r0[..., i1], r1[..., i0], r1[..., i1]
        w0, w1, h0, h1 = l0[None, None, None, :], l1[None, None, None, :], l0[None, None, :, None], l1[None, None, :, None]
        v = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
    return 2 * v - 1 if normalize else v


INPUT_SHAPES = [(1, 3, 256, 256), (2, 3, 512, 512), (1, 3, 1024, 1024), (1, 3, 299, 299)]


@pytest.mark.parametrize('normalize', [True, False], ids=['normalized', 'plain'])
@pytest.mark.parametrize('shape', INPUT_SHAPES, ids=[str(s[0]) + 'x' + str(s[2]) for s in INPUT_SHAPES])
def test_inception_input_kernel(shape, normalize):
    """The raw entry point writes [B, 299, 299, 3] between guards from a source whose never-tapped pixels are NaN: finite
    everywhere, bit for bit the header's formula in fp32 torch ops, and within 2^-22 * max|x| of F.interpolate on the
    GPU (three roundings per form, two forms; with normalize_input twice that, plus the final rounding of 2v - 1 in
    each form); whether the latter two are bit-equal is printed."""
    L = lib()
    b, _, s, _ = shape
    x = synth.tensor(f'fid_gpu/input/{b}x{s}', shape, dist='uniform').to(dev())
    assert L.fmgan_inception_input_select(b, s, s) == (2 if s == 299 else 1)
    src = x.clone()
    if s != 299:
        i0, i1, _, _ = _taps(s, dev())
        tapped = torch.zeros(s, dtype=torch.bool, device=dev())
        tapped[i0] = True
        tapped[i1] = True
        never = ~(tapped[:, None] & tapped[None, :])
        src[:, :, never] = float('nan')
        print(f'{s}: {int(never.sum())} of {s * s} pixels are never tapped')
        assert (s == 1024) == (int(never.sum()) > 0)      # below a ratio of 2 every source pixel is a tap
    buf, out = guarded((b, 299, 299, 3))
    assert L.fmgan_inception_input_f32(src.data_ptr(), out.data_ptr(), b, s, s, int(normalize), _stream()) == 0
    got = out.permute(0, 3, 1, 2)
    assert guards_intact(buf) and bool(torch.isfinite(got).all())
    assert torch.equal(got, _formula(x, normalize))
    ref = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False) if s != 299 else x
    ref = 2 * ref - 1 if normalize else ref
    diff = float((got - ref).abs().max())
    print(f'{s} normalize={normalize}: max |kernel - F.interpolate| {diff:.3e}, bit-equal {bool(torch.equal(got, ref))}')
    bound = 2.0 ** -22 * float(x.abs().max())
    if normalize:       # 2v - 1 doubles the difference of v and rounds once in either form (relative 2^-24 each)
        bound = 2 * bound + 2 * 2.0 ** -24 * float(ref.abs().max())
    assert diff <= bound


def test_inception_input_wrapper_paths():
    """op.inception_input: one launch where the kernel serves, channels_last result equal to the raw kernel's; a 300^2
    image goes to the composite (no launch), as does fuse=False."""
    from op import inception_input as II
    x = synth.tensor('fid_gpu/input/wrapper', (2, 3, 256, 256), dist='uniform').to(dev())
    with observed() as rec:
        y = II.inception_input(x, normalize_input=True)
    assert rec.count('inception_input') == 1 and II.inception_input_serves(x)
    assert tuple(y.shape) == (2, 3, 299, 299) and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, _formula(x, True))
    odd = synth.tensor('fid_gpu/input/odd', (1, 3, 300, 300), dist='uniform').to(dev())
    with observed() as rec:
        z = II.inception_input(odd, normalize_input=False)
        w = II.inception_input(x, normalize_input=True, fuse=False)
    assert rec.count('inception_input') == 0 and not II.inception_input_serves(odd)
    assert torch.equal(z, F.interpolate(odd, size=(299, 299), mode='bilinear', align_corners=False))
    # the kernel test's bound with normalize_input: twice 2^-22 max|x|, and the rounding of 2v - 1 in each form
    assert float((w - y).abs().max()) <= 2.0 ** -21 * float(x.abs().max()) + 2 * 2.0 ** -24 * float(w.abs().max())
    with pytest.raises(RuntimeError, match='inference only'):
        II.inception_input(x.clone().requires_grad_(True))


# ------------------------------------------------------------------------------------------------ the loop, the network
@pytest.mark.parametrize('fuse', [True, False], ids=['fused', 'composite'])
def test_sample_statistics_on_generator_matches_reference(golden, fuse):
    """Sample_Statistics with Generator(64) (tests/synth.py's weights, stored noise) and the stand-in inception, batches
    of 32 and 38 with fixed latents, against the reference's FID of the same pipeline on the CPU, within 10 x the
    reference's own spread (tests/fid_cases.py)."""
    import stylegan2
    from Evaluation import fid as FID
    c = fc.SAMPLE_BY_NAME['g64']
    g = golden('fid')
    gen = fc.Pinned(load(stylegan2.Generator(c['size'], 512, 8), 'generator', 4))
    inc = fc.StandinInception().to(dev())
    real = fc.real_stats()
    with observed() as rec:
        stats = FID.Sample_Statistics(gen, inc, 1, None, c['batch'], c['n_sample'], dev(), sampler=fc.sampler(c), fuse=fuse)
    assert rec.count('fid_stats') == (2 if fuse else 0) and stats.count == 70
    got = FID.calc_fid(*stats.finish(), real['mean'], real['cov'])
    want, tol = float(g['sample_g64/fid']), fc.tolerance(g, 'sample_g64')
    print(f'g64 fuse={fuse}: fid {got!r} reference {want!r} |diff| {abs(got - want):.3e} tolerance {tol:.3e}')
    assert abs(got - want) <= tol


def test_sample_statistics_does_not_synchronise():
    """The loop, the updates and finish() under torch.cuda.set_sync_debug_mode('error'), which turns any host
    synchronisation into an error (the reference copies every batch's features to the host): latents already on the
    device, the toy generator and the stand-in inception, batches of 32 and 38 through the kernel."""
    from Evaluation import fid as FID
    c = fc.SAMPLE_BY_NAME['toy']
    gen, inc = fc.ToyGenerator().to(dev()), fc.StandinInception().to(dev())
    z = [fc.latents(c, i, b).to(dev()) for i, b in enumerate(FID.batch_split(c['n_sample'], c['batch']))]
    probe = torch.ones(1, device=dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.item()                     # the mode is live in this build
        with observed() as rec:
            stats = FID.Sample_Statistics(gen, inc, 1, None, c['batch'], c['n_sample'], dev(),
                                          sampler=lambda i, b, dim, device: z[i], fuse=True)
            mean, cov = stats.finish()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert rec.count('fid_stats') == 3 and stats.count == 70
    assert bool(torch.isfinite(mean).all()) and torch.equal(cov, cov.T)


# module-by-module forward on the GPU against the same network in float64 on the CPU, max |diff| / max |out| of the
# [2, 2048] features, measured with tools/bench_fid.py --inception-error on an MI355X
MODULES_GPU_VS_F64 = 1.49e-6


def test_inception_folded_fused_forward_on_gpu():
    """InceptionV3() with its own initialisation at [2, 3, 256, 256]: the folded, fused forward against the
    module-by-module forward on the GPU, relative to the output's max.  The margin is that of fp32 convolution
    reassociation through 94 layers: 4 x the module-by-module GPU-versus-CPU-float64 difference (MODULES_GPU_VS_F64).
    Measured on an MI355X (tools/bench_fid.py --inception-error): modules on the GPU against float64 on the CPU 1.49e-6,
    folded + fused against modules on the GPU 1.56e-6; allowed here 5.96e-6."""
    from Evaluation.inception import InceptionV3
    torch.manual_seed(0)
    m = InceptionV3().to(dev()).eval()
    x = ((synth.tensor('fid_gpu/inception/x', (2, 3, 256, 256), dist='uniform') + 1) / 2).to(dev())
    with torch.no_grad(), observed() as rec:
        a = m(x)[0]
        b = m.forward_modules(x)[0]
    assert rec.count('inception_input') == 1
    assert tuple(a.shape) == (2, 2048, 1, 1) and bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0
    rel = float((a - b).abs().max()) / float(b.abs().max())
    print(f'folded + fused against modules: max |diff| / max |out| {rel:.3e}; allowed {4 * MODULES_GPU_VS_F64:.3e}')
    assert rel <= 4 * MODULES_GPU_VS_F64
