"""CPU tests of the perceptual path length (Evaluation/ppl.py), its input stage's host logic (op/ppl_input.py,
fmgan_lpips_pair_input_select) and lpips' forward_scaled: everything here runs without a device.  The kernel itself and
the Generator cases are in tests/test_ppl_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import codeobj
import ppl_cases as pc
import synth
from nets import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED, EOVERFLOW = 0, -1, -2, -4


# ------------------------------------------------------------------------------------------------ library and binding
def test_library_exports_the_pair_input_entry_points():
    """Both symbols are exported, declared in the header, and bound in op/_native/core.py's table with the header's argument
    counts (eight ints; five pointers, eight ints and the stream)."""
    hdr = open(os.path.join(ROOT, 'include', 'fmgan_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    L = lib()
    for name, pointers, ints in (('fmgan_lpips_pair_input_select', 0, 8), ('fmgan_lpips_pair_input_f32', 6, 8)):
        params = re.search(r'\b' + name + r'\s*\(([^()]*)\)\s*;', hdr).group(1).split(',')
        assert len(params) == pointers + ints and sum('*' in p for p in params) == pointers, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert sum(t is ctypes.c_void_p for t in fn.argtypes) == pointers, name
        assert sum(t is ctypes.c_int for t in fn.argtypes) == ints and fn.restype is ctypes.c_int, name
    assert L.fmgan_abi_version() == 1


def test_select_returns_a_kernel_id_or_the_launch_status():
    """fmgan_lpips_pair_input_select is the launch's plan with the launch left out: f for the vector form (ow % 4 == 0),
    8 + f for the bounded one, and for each refused argument class the status the launch itself returns (the launches here
    are refused before any HIP call: the pointers are placeholders)."""
    L = lib()
    sel = L.fmgan_lpips_pair_input_select
    fake = ctypes.c_void_p(0x1000)

    def run(*args):
        return L.fmgan_lpips_pair_input_f32(fake, fake, fake, fake, fake, *args, None)
    served = {(8, 1024, 1024, 0, 0, 1024, 1024, 4): 4, (8, 1024, 1024, 384, 256, 512, 512, 2): 2,
              (64, 256, 256, 0, 0, 256, 256, 1): 1, (1, 512, 512, 192, 128, 256, 256, 1): 1,
              (1, 5, 7, 0, 0, 5, 7, 1): 9, (3, 12, 20, 0, 0, 12, 20, 2): 10, (1, 16, 24, 4, 3, 8, 20, 4): 12,
              (1, 16, 24, 0, 0, 16, 24, 4): 12, (1, 32, 32, 12, 8, 16, 16, 1): 1}
    for args, kernel in served.items():
        assert sel(*args) == kernel, args
    refused = {
        EINVAL: [(0, 64, 64, 0, 0, 64, 64, 1), (-1, 64, 64, 0, 0, 64, 64, 1), (1, 0, 64, 0, 0, 64, 64, 1),
                 (1, 64, 64, -1, 0, 64, 64, 1), (1, 64, 64, 0, 0, 0, 64, 1), (1, 64, 64, 1, 0, 64, 64, 1),
                 (1, 64, 64, 0, 8, 64, 60, 1), (1, 64, 64, 0, 0, 64, 2147483647, 1),
                 (1, 64, 64, 0, 0, 66, 64, 3)],                                   # outside the image comes first
        EUNSUPPORTED: [(1, 64, 64, 0, 0, 64, 64, 3), (1, 64, 64, 0, 0, 64, 64, 8), (1, 64, 64, 0, 0, 64, 64, 0),
                       (1, 64, 64, 0, 0, 62, 64, 4), (1, 64, 64, 0, 0, 64, 63, 2), (1, 16, 24, 4, 3, 8, 18, 4)],
        EOVERFLOW: [(1, 65536, 65536, 0, 0, 65536, 65536, 1), (1, 46341, 46341, 0, 0, 4, 4, 1),
                    (1 << 30, 64, 64, 0, 0, 64, 64, 1), (1 << 29, 256, 256, 0, 0, 256, 256, 1)],
    }
    for status, rows in refused.items():
        for args in rows:
            assert sel(*args) == status, (status, args)
            assert run(*args) == status, (status, args)
    # null pointers are the launch's alone; they come before the plan
    good = (1, 64, 64, 0, 0, 64, 64, 1)
    for k in range(5):
        ptrs = [fake] * 5
        ptrs[k] = None
        assert L.fmgan_lpips_pair_input_f32(*ptrs, *good, None) == EINVAL, k
    assert L.fmgan_lpips_pair_input_f32(None, None, None, None, None, 1, 64, 64, 0, 0, 64, 64, 3, None) == EINVAL


GEOMETRY = [
    # size, crop -> (window (y0, x0, hc, wc), f) or None (the composite)
    (64, False, ((0, 0, 64, 64), 1)), (64, True, ((24, 16, 32, 32), 1)),
    (256, False, ((0, 0, 256, 256), 1)), (256, True, ((96, 64, 128, 128), 1)),
    (512, False, ((0, 0, 512, 512), 2)), (512, True, ((192, 128, 256, 256), 1)),
    (768, False, None), (768, True, ((288, 192, 384, 384), 1)),
    (1024, False, ((0, 0, 1024, 1024), 4)), (1024, True, ((384, 256, 512, 512), 2)),
]


@pytest.mark.parametrize('size,crop,want', GEOMETRY, ids=lambda v: str(v) if isinstance(v, (int, bool)) else '')
def test_pair_input_geometry_is_the_references(size, crop, want):
    """The window and the factor are the reference's (c = S // 8, rows 3c:7c, columns 2c:6c; factor = S' // 256, a
    reduction only when factor > 1), written out by hand above; the kernel's plan is that window at f = factor for exact
    reductions by 2 and 4, f = 1 where nothing is resampled, and nothing for S' = 768; the library plans the vector form
    for each.  A CPU tensor is never served."""
    from op import ppl_input as PI
    window, factor = PI.pair_geometry(size, size, crop)
    c = size // 8
    assert window == ((3 * c, 2 * c, 4 * c, 4 * c) if crop else (0, 0, size, size)) and factor == window[2] // 256
    plan = PI.pair_input_plan((4, 3, size, size), crop)
    assert plan == want
    if plan is not None:
        (y0, x0, hc, wc), f = plan
        assert lib().fmgan_lpips_pair_input_select(2, size, size, y0, x0, hc, wc, f) == f
        assert (hc // f, wc // f) == ((256, 256) if factor > 1 else (hc, wc))
    for shape in ((3, 3, size, size), (0, 3, size, size), (4, 1, size, size), (4, 3, size, size // 2), (4, 3, size)):
        assert PI.pair_input_plan(shape, crop) is None, shape
    assert not PI.pair_input_serves(torch.zeros(2, 3, 8, 8), crop)


# ------------------------------------------------------------------------------------------------ lpips.forward_scaled
def test_forward_scaled_equals_forward_bit_for_bit():
    import lpips
    percept = lpips.PerceptualLoss(model='net-lin', net='vgg')
    percept.load_state_dict(pc.percept_state_dict(percept.state_dict()))
    a = synth.tensor('ppl/fs/a', (2, 3, 32, 32), dist='uniform')
    b = synth.tensor('ppl/fs/b', (2, 3, 32, 32), dist='uniform')
    scaling = percept.net.scaling_layer
    with torch.no_grad():
        d = percept(a, b)
        assert tuple(d.shape) == (2, 1, 1, 1) and bool((d > 0).all())
        assert torch.equal(percept.forward_scaled(scaling(a), scaling(b)), d)
        assert torch.equal(percept.net.forward_scaled(scaling(b), scaling(a)), d)        # net(target, pred)
        assert torch.equal(percept.net(b, a), d)
        sa = scaling(a)
        assert torch.count_nonzero(percept.net.forward_scaled(sa, sa)) == 0
        assert torch.count_nonzero(percept(a, a)) == 0


# ------------------------------------------------------------------------------------------------ composite
def test_composite_against_interpolate():
    """pair_input_composite without scaling at [2, 3, 512, 512] is the two halves of F.interpolate's 256^2 image.  Gate
    2^-22 * max|x|: each form rounds three times at magnitudes <= max|x| (two sums of a row pair or column pair, then
    their sum), each rounding <= 2^-24 * max|x|, two of them halved afterwards: <= 2^-23 * max|x| per form, and two
    forms.  With the ScalingLayer it is the module applied to those halves; both outputs are channels_last."""
    import lpips
    from op import ppl_input as PI
    x = synth.tensor('ppl/composite/x', (2, 3, 512, 512), dist='uniform')
    want = F.interpolate(x, size=(256, 256), mode='bilinear', align_corners=False)
    got = PI.pair_input_composite(x, None)
    gate = 2.0 ** -22 * float(x.abs().max())
    for g, w in zip(got, (want[::2], want[1::2])):
        assert tuple(g.shape) == (1, 3, 256, 256) and g.is_contiguous(memory_format=torch.channels_last)
        err = float((g - w).abs().max())
        print('composite against F.interpolate: max|d|', err, 'gate', gate, 'bit-equal', torch.equal(g, w))
        assert err <= gate
    scaling = lpips.ScalingLayer()
    scaled = PI.pair_input_composite(x, scaling)
    assert torch.equal(scaled[0], scaling(got[0])) and torch.equal(scaled[1], scaling(got[1]))
    # a CPU tensor goes to the composite whatever `fuse` says; the crop keeps rows 3c:7c, columns 2c:6c
    y = synth.tensor('ppl/composite/y', (4, 3, 64, 64), dist='uniform')
    for fuse in (True, False):
        a0, a1 = PI.pair_input(y, scaling, crop=True, fuse=fuse)
        assert torch.equal(a0, scaling(y[::2, :, 24:56, 16:48])) and torch.equal(a1, scaling(y[1::2, :, 24:56, 16:48]))
    z = synth.tensor('ppl/composite/z', (2, 3, 768, 768), dist='uniform').double()
    b0, b1 = PI.pair_input(z, scaling.double())
    assert b0.dtype == torch.float64 and tuple(b0.shape) == tuple(b1.shape) == (1, 3, 256, 256)
    with pytest.raises(RuntimeError, match='inference only'):
        PI.pair_input(y.clone().requires_grad_(True), scaling)


# ------------------------------------------------------------------------------------------------ Evaluation/ppl.py
def test_toy_case_matches_the_reference(golden):
    """The `toy` case through PPL_Distances / Get_PPL_Score on the CPU against the reference's float64 run: per pair
    |d - dist64| <= 4 * max over pairs |dist32 - dist64| (the project's rule for an fp32 path against the reference's own
    fp32 error), the same pairs survive the percentile filter (two dropped at each end), and the score within the same
    gate."""
    from Evaluation import ppl as P
    g = golden('ppl')
    c = pc.BY_NAME['toy']
    gen = pc.ToyGenerator(c['latent_dim'])
    args = (c['n_sample'], c['batch'], c['eps'], c['latent_dim'], 'cpu')
    d = P.PPL_Distances(gen, pc.standin_distance, *args, sampler=pc.sampler(c))
    assert tuple(d.shape) == (256,) and d.dtype == torch.float32
    d = d.double().numpy()
    d32, d64 = g['toy/dist'], g['toy/dist64']
    gate = 4 * np.abs(d32 - d64).max()
    print('toy: max|d - dist64|', np.abs(d - d64).max(), 'gate', gate)
    assert np.all(np.abs(d - d64) <= gate)

    def kept(v):
        lo, hi = np.percentile(v, 1, method='lower'), np.percentile(v, 99, method='higher')
        return np.logical_and(lo <= v, v <= hi)
    assert np.array_equal(kept(d), kept(d64)) and int(kept(d).sum()) == 252
    score = P.Get_PPL_Score(gen, *args, None, percept=pc.standin_distance, sampler=pc.sampler(c))
    assert isinstance(score, np.float64)
    print('toy: score', score, 'reference', float(g['toy/score']), float(g['toy/score64']))
    assert abs(score - float(g['toy/score64'])) <= gate
    assert score == P.PPL_Filter(torch.from_numpy(d).float())
    # behind a wrapper with .module the mapping network is the wrapped generator's; the latents are the reference's
    wrapped = torch.nn.Module()
    wrapped.module = gen
    wrapped.forward = lambda **kw: gen(**kw)
    again = P.PPL_Distances(wrapped, pc.standin_distance, 64, 64, c['eps'], c['latent_dim'], 'cpu', sampler=pc.sampler(c))
    assert np.array_equal(again.double().numpy(), d[:64])
    z, t = pc.inputs(c, 0)
    lat = P.Interpolated_Latents(gen.style.double(), z.double(), t.double(), c['eps'])
    np.testing.assert_allclose(lat.numpy(), g['toy/latent_e64'], rtol=1e-12, atol=1e-12)
    # normalize divides by eps^2 (the script half of the reference's file)
    norm = P.PPL_Distances(gen.float(), pc.standin_distance, 64, 64, c['eps'], c['latent_dim'], 'cpu',
                           sampler=pc.sampler(c), normalize=True)
    assert torch.equal(norm, again / (c['eps'] ** 2))


def test_batch_schedule_and_value_error():
    """n_sample // batch_size batches of batch_size pairs (the reference's residual is never used): 10 samples at batch 4
    give 8 distances; fewer samples than one batch is a ValueError.  The default sampler draws randn then rand."""
    from Evaluation import ppl as P
    gen = pc.ToyGenerator(16)
    seen = []

    def sampler(idx, batch, dim, device):
        seen.append((idx, batch, dim, device))
        return P.default_sampler(idx, batch, dim, device)
    d = P.PPL_Distances(gen, pc.standin_distance, 10, 4, 1e-2, 16, 'cpu', sampler=sampler)
    assert tuple(d.shape) == (8,) and seen == [(0, 4, 16, 'cpu'), (1, 4, 16, 'cpu')]
    assert bool(torch.isfinite(d).all()) and bool((d > 0).all())
    for n in (3, 0):
        with pytest.raises(ValueError):
            P.PPL_Distances(gen, pc.standin_distance, n, 4, 1e-2, 16, 'cpu')
    with pytest.raises(ValueError):
        P.Get_PPL_Score(gen, 3, 4, 1e-2, 16, 'cpu', None, percept=pc.standin_distance)
    torch.manual_seed(11)
    z, t = P.default_sampler(0, 4, 16, 'cpu')
    torch.manual_seed(11)
    assert torch.equal(z, torch.randn([8, 16])) and torch.equal(t, torch.rand(4))
    assert tuple(P.PPL_Distances(gen, pc.standin_distance, 4, 4, 1e-2, 16, 'cpu').shape) == (4,)


# ------------------------------------------------------------------------------------------------ kernel resources
@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    """The notes of the pair-input kernels in the built library, read as tests/test_lpips_kernel_budget.py reads them."""
    notes = codeobj.kernel_notes(tmp_path_factory.mktemp('codeobj'))
    return {name: k for name, k in notes.items() if 'lpips_pair_input' in name}


def test_pair_input_kernels_have_no_spill_and_no_scratch(kernels):
    """Six instantiations (f = 1, 2, 4; vector and bounded form); none spills or uses scratch: the kernel is HBM-bound
    and a spill would put its loads back into memory.  64 registers keep eight waves per SIMD."""
    assert len(kernels) == 6, sorted(kernels)
    for f in (1, 2, 4):
        assert sum(f'ILi{f}ELb1' in k for k in kernels) == 1 and sum(f'ILi{f}ELb0' in k for k in kernels) == 1, f
    for name, k in sorted(kernels.items()):
        print(name, k)
        assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0, (name, k)
        assert k['vgpr'] <= 64, (name, k)
