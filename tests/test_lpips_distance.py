"""LPIPS distance of one VGG tap on its kernel (csrc/lpips_distance.hip, op/lpips_distance.py) and its use in
lpips.PNetLin and the G step.

Reference: the composite of lpips/__init__.py (unit-normalise over channels, squared difference, 1x1 conv, spatial mean)
in float64 on the CPU, differentiated by autograd.  Gate (the form tests/test_hip_modconv_bf16.py uses for the
split-operand kernel): with err(x) = max|x - ref64| / max|ref64|,

    err(kernel) <= 2 * err(fp32 composite on the GPU, same inputs) + 2e-6

for the distance and for each gradient tensor; both errors are printed.

Inputs: ReLU-like features relu(N(0.3, 1)) (the smallest pixel norm over the shapes below is 3.96 on the CPU: no pixel
is near zero except where a test zeroes one), |U(-1, 1)| weights, one upstream gradient per sample (distinct; a negative
one and a zero among them).

CPU: the host logic of the three entry points through ctypes (block sizing rule: ceil(H*W / pixels per block step) blocks
per sample, at most ceil(8 * 256 CUs / batch) and at most 1024), their statuses, the header, the fall-back decisions.
"""
import copy
import ctypes
import functools
import os
import re

import pytest
import torch

import launches
import synth
from gpumem import dev, misaligned_nhwc
from nets import PinNoise, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-10
GRADS = (-0.75, 0.0, 1.5)


def composite(f0, f1, w, eps=EPS):
    """PNetLin.forward's lines for one tap, restated: works in any dtype on any device."""
    u0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + eps)
    u1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + eps)
    return torch.nn.functional.conv2d((u0 - u1) ** 2, w).mean([2, 3], keepdim=True)


def upstream(n):
    return torch.tensor(GRADS[:n] if n > 1 else [1.5]).view(n, 1, 1, 1)


def nhwc(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def err(x, ref, mask=None):
    x, ref = x.detach().cpu().double(), ref.detach().cpu().double()
    if mask is not None:
        x, ref = x[mask], ref[mask]
    return float((x - ref).abs().max() / ref.abs().max())


def gate(what, e_kernel, e_fp32):
    print(f'{what}: err(kernel) {e_kernel:.3e}  err(fp32 composite, GPU) {e_fp32:.3e}')
    assert e_kernel <= 2 * e_fp32 + 2e-6, (what, e_kernel, e_fp32)


def observed(fn):
    """(fn(), the infos of the lpips_distance launches during it)."""
    with launches.observed() as rec:
        out = fn()
    return out, rec.infos('lpips_distance')


def make_inputs(shape, zero_pixel=None):
    name = 'lpd/' + 'x'.join(map(str, shape))
    f0 = torch.relu(synth.tensor(name + '/f0', shape, shift=0.3))
    f1 = torch.relu(synth.tensor(name + '/f1', shape, shift=0.3))
    if zero_pixel is not None:
        n, y, x = zero_pixel
        f1[n, :, y, x] = 0.0
    w = synth.tensor(name + '/w', (1, shape[1], 1, 1), dist='uniform').abs()
    return f0, f1, w, upstream(shape[0])


def differentiate(fn, f0, f1, w, g):
    """(d, grad_f0, grad_f1) of fn(f0, f1, w) with both features as leaves."""
    a, b = f0.detach().requires_grad_(True), f1.detach().requires_grad_(True)
    d = fn(a, b, w)
    d.backward(g.to(d))
    return d.detach(), a.grad, b.grad


@functools.lru_cache(maxsize=None)
def case(shape, zero_pixel=None):
    """Inputs, the float64 CPU reference and the fp32 composite on the GPU for one shape: computed once, shared."""
    f0, f1, w, g = make_inputs(shape, zero_pixel)
    ref = differentiate(composite, f0.double(), f1.double(), w.double(), g.double())
    c0, c1, cw, cg = nhwc(f0), nhwc(f1), w.to(dev()), g.to(dev())
    f32 = differentiate(composite, c0, c1, cw, cg)
    return dict(f0=c0, f1=c1, w=cw, g=cg, ref=ref, f32=f32)


def kernel_backward(c, need0, need1):
    from op.lpips_distance import lpips_distance
    a, b = c['f0'].detach().requires_grad_(need0), c['f1'].detach().requires_grad_(need1)
    d = lpips_distance(a, b, c['w'])
    d.backward(c['g'])
    return d.detach(), a.grad, b.grad


# ------------------------------------------------------------------------------------------------------------- CPU
def test_blocks_is_host_logic():
    """fmgan_lpips_distance_blocks without a device: ceil(hw / pixels per block step) blocks per sample (16 pixels x
    4 / 2 / 1 / 1 per lane at C = 64 / 128 / 256 / 512), at most ceil(2048 / batch) (8 blocks per CU over the batch,
    256 CUs assumed without a device) and at most 1024; 0 where the kernel does not serve."""
    L = lib()
    assert L.fmgan_lpips_distance_blocks(8, 64, 1 << 20) == 2048 // 8
    assert L.fmgan_lpips_distance_blocks(8, 512, 128 * 128) == 2048 // 8
    assert L.fmgan_lpips_distance_blocks(1, 64, 1 << 20) == 1024                 # the cap
    assert L.fmgan_lpips_distance_blocks(3, 64, 35) == 1 and L.fmgan_lpips_distance_blocks(1, 64, 1) == 1
    assert L.fmgan_lpips_distance_blocks(2, 64, 67 * 129) == -(-67 * 129 // 64)
    assert L.fmgan_lpips_distance_blocks(2, 128, 54) == 2 and L.fmgan_lpips_distance_blocks(2, 256, 20) == 2
    assert L.fmgan_lpips_distance_blocks(2, 512, 9) == 1 and L.fmgan_lpips_distance_blocks(2, 512, 17) == 2
    assert L.fmgan_lpips_distance_blocks(2, 96, 64) == 0
    assert L.fmgan_lpips_distance_blocks(0, 64, 64) == 0 and L.fmgan_lpips_distance_blocks(2, 64, 0) == 0
    assert L.fmgan_lpips_distance_blocks(65536, 64, 64) == 0                     # grid.y
    assert L.fmgan_lpips_distance_blocks(1, 512, 1 << 21) == 0                   # 32-bit offsets inside a sample
    assert L.fmgan_lpips_distance_blocks(1, 512, (1 << 21) - 1) == 1024


def test_statuses_before_any_hip_call():
    L = lib()
    fwd, bwd = L.fmgan_lpips_distance_f32, L.fmgan_lpips_distance_backward_f32
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    assert fwd(None, None, None, None, 0, 64, 64, EPS, None) == 0                 # empty batch: nothing to do
    assert bwd(None, None, None, None, None, None, 0, 64, 64, EPS, None) == 0
    assert fwd(None, p, p, p, 2, 64, 64, EPS, None) == -1 and fwd(p, p, p, None, 2, 64, 64, EPS, None) == -1
    assert fwd(p, p, p, p, 2, 64, 0, EPS, None) == -1 and fwd(p, p, p, p, -1, 64, 64, EPS, None) == -1
    assert fwd(p, p, p, p, 2, 0, 64, EPS, None) == -1
    assert bwd(p, p, p, None, p, p, 2, 64, 64, EPS, None) == -1                   # no upstream gradient
    assert bwd(p, p, p, p, None, None, 2, 64, 64, EPS, None) == -1                # neither gradient wanted
    assert bwd(p, p, p, p, p, p, 2, 64, -3, EPS, None) == -1
    assert fwd(p, p, p, p, 2, 96, 64, EPS, None) == -2 and bwd(p, p, p, p, p, None, 2, 96, 64, EPS, None) == -2
    assert fwd(p, odd, p, p, 2, 64, 64, EPS, None) == -2 and fwd(p, p, odd, p, 2, 64, 64, EPS, None) == -2
    assert bwd(p, p, p, p, None, odd, 2, 64, 64, EPS, None) == -2
    assert fwd(p, p, p, p, 65536, 64, 64, EPS, None) == -4 and bwd(p, p, p, p, p, p, 65536, 64, 64, EPS, None) == -4
    assert fwd(p, p, p, p, 1, 512, 1 << 21, EPS, None) == -4
    assert L.fmgan_abi_version() == 1


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'fmgan_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('fmgan_lpips_distance_blocks', 'fmgan_lpips_distance_f32', 'fmgan_lpips_distance_backward_f32'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert hasattr(lib(), name)


def test_cpu_tensors_keep_the_composite():
    """The switch exists and is on by default; CPU features are never served, PNetLin's value on them is the composite's;
    the raw binding refuses them."""
    import lpips
    from op import _native, lpips_distance, lpips_distance_serves
    assert lpips.FUSED is (os.environ.get('FMGAN_LPIPS_FUSED', '1') != '0')
    f0, f1, w, _ = make_inputs((2, 64, 5, 7))
    f0, f1 = (t.contiguous(memory_format=torch.channels_last) for t in (f0, f1))
    assert not lpips_distance_serves(f0, f1, w)
    _, obs = observed(lambda: lpips_distance(f0, f1, w))
    assert obs == []
    assert torch.equal(lpips_distance(f0, f1, w), composite(f0, f1, w))
    with pytest.raises(RuntimeError):
        _native.lpips_distance(f0, f1, w)
    with pytest.raises(ValueError):
        _native.lpips_distance(f0.contiguous(), f1.contiguous(), w)                # NCHW: refused by layout
    with pytest.raises(ValueError):
        _native.lpips_distance(f0, f1[:1], w)


# ------------------------------------------------------------------------------------------------------------- GPU
# (3,64,5,7): 35 pixels, a ragged tail; the next three: the other channel counts; one pixel; several blocks per sample
# (order of the partial sums); the last two make a block walk the grid-stride loop more than once (blocks at the cap).
SHAPES = [(3, 64, 5, 7), (2, 128, 9, 6), (2, 256, 4, 5), (2, 512, 3, 3), (1, 64, 1, 1), (2, 64, 67, 129),
          (1, 64, 257, 257), (1, 512, 129, 129)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def _blocks(shape):
    n, c, h, w = shape
    return lib().fmgan_lpips_distance_blocks(n, c, h * w)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_matches_fp64_composite(shape):
    from op.lpips_distance import lpips_distance, lpips_distance_serves
    c = case(shape)
    if shape == (2, 64, 67, 129):
        assert _blocks(shape) > 1
    if shape[2] > 128:
        assert _blocks(shape) == 1024 and shape[2] * shape[3] > 1024 * 16 * max(1, 256 // shape[1])
    assert lpips_distance_serves(c['f0'], c['f1'], c['w'])
    (d, obs) = observed(lambda: lpips_distance(c['f0'], c['f1'], c['w']))
    n, ch, h, w = shape
    assert obs == [(n, ch, h * w, 0)]
    assert d.shape == (n, 1, 1, 1) and d.dtype == torch.float32
    gate(f'd {shape}', err(d, c['ref'][0]), err(c['f32'][0], c['ref'][0]))
    assert torch.equal(lpips_distance(c['f0'], c['f1'], c['w']), d)                       # run to run: the same bits
    assert torch.equal(lpips_distance(c['f1'], c['f0'], c['w']), d)                       # (u0 - u1)^2 is symmetric
    assert torch.count_nonzero(lpips_distance(c['f0'], c['f0'].clone(), c['w'])) == 0     # d(f, f) = 0 exactly


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_backward_matches_fp64_autograd(shape):
    c = case(shape)
    n, ch, h, w = shape
    for need0, need1 in ((False, True), (True, False), (True, True)):
        (out, obs) = observed(lambda: kernel_backward(c, need0, need1))
        assert obs == [(n, ch, h * w, 0), (n, ch, h * w, 1)]
        again = kernel_backward(c, need0, need1)
        for k, need in ((1, need0), (2, need1)):
            if not need:
                assert out[k] is None
                continue
            assert out[k].shape == shape and out[k].permute(0, 2, 3, 1).is_contiguous()
            gate(f'grad_f{k - 1} {shape} needs=({int(need0)},{int(need1)})', err(out[k], c['ref'][k]),
                 err(c['f32'][k], c['ref'][k]))
            assert torch.equal(out[k], again[k])
            for s in range(n):
                if float(c['g'][s]) == 0.0:
                    assert torch.count_nonzero(out[k][s]) == 0                            # upstream 0: an all-zero gradient


@pytest.mark.gpu
def test_zero_norm_pixel_is_nan_there_and_nowhere_else():
    """One pixel of f1 exactly zero: autograd's composite gives NaN for that pixel's grad_f1 (sqrt backward, 0/0), and
    so does the kernel; no other position is touched, the distance and grad_f0 stay finite."""
    shape, pixel = (2, 64, 5, 7), (0, 2, 3)
    c = case(shape, pixel)
    d, g0, g1 = kernel_backward(c, True, True)
    gate('d zero-norm', err(d, c['ref'][0]), err(c['f32'][0], c['ref'][0]))
    there = torch.zeros(shape, dtype=torch.bool)
    there[pixel[0], :, pixel[1], pixel[2]] = True
    assert torch.equal(~torch.isfinite(g1).cpu(), there)
    assert torch.equal(~torch.isfinite(c['f32'][2]).cpu(), there)                         # as the fp32 composite on the GPU
    assert torch.equal(~torch.isfinite(c['ref'][2]), there)
    gate('grad_f1 zero-norm, other positions', err(g1, c['ref'][2], ~there), err(c['f32'][2], c['ref'][2], ~there))
    assert torch.isfinite(g0).all()
    gate('grad_f0 zero-norm', err(g0, c['ref'][1]), err(c['f32'][1], c['ref'][1]))


@pytest.mark.gpu
def test_unserved_calls_fall_back_to_the_composite():
    from op import _native
    from op.lpips_distance import lpips_distance, lpips_distance_serves
    c = case((3, 64, 5, 7))
    f0, f1, w = c['f0'], c['f1'], c['w']
    f96 = nhwc(torch.relu(synth.tensor('lpd/96/f0', (2, 96, 5, 7), shift=0.3)))
    g96 = nhwc(torch.relu(synth.tensor('lpd/96/f1', (2, 96, 5, 7), shift=0.3)))
    w96 = synth.tensor('lpd/96/w', (1, 96, 1, 1), dist='uniform').abs().to(dev())
    calls = {
        'nchw': (f0.contiguous(), f1.contiguous(), w),
        'c96': (f96, g96, w96),
        'offset': (misaligned_nhwc(f0), f1, w),
        'bf16': (f0.bfloat16(), f1.bfloat16(), w.bfloat16()),
        'weight_grad': (f0, f1, w.clone().requires_grad_(True)),
    }
    for name, (a, b, ww) in calls.items():
        assert not lpips_distance_serves(a, b, ww), name
        (d, obs) = observed(lambda: lpips_distance(a, b, ww))
        assert obs == [], name
        assert torch.equal(d, composite(a, b, ww)), name
    d = lpips_distance(*calls['weight_grad'])
    d.sum().backward()
    assert calls['weight_grad'][2].grad is not None                                       # the composite's autograd
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert not lpips_distance_serves(f0, f1, w)
    with pytest.raises(RuntimeError, match='float32'):
        _native.lpips_distance(f0.bfloat16(), f1.bfloat16(), w)
    with pytest.raises(RuntimeError, match='float32'):
        _native.lpips_distance_backward(f0.double(), f1.double(), w.double(), c['g'], False, True)


@pytest.mark.gpu
def test_no_host_synchronisation():
    from op.lpips_distance import lpips_distance
    c = case((3, 64, 5, 7))
    a, b = c['f0'].detach().requires_grad_(True), c['f1'].detach().requires_grad_(True)
    probe = torch.ones(1, device=dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.item()                     # the mode is live in this build
        lpips_distance(a, b, c['w']).backward(c['g'])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert a.grad is not None and b.grad is not None


def _perceptual(seed=0):
    import lpips
    torch.manual_seed(seed)
    return lpips.PerceptualLoss(model='net-lin', net='vgg')


def _module_run(m, pred, target, g, fused):
    import lpips
    old = lpips.FUSED
    lpips.FUSED = fused
    try:
        p = pred.detach().requires_grad_(True)
        d = m(p, target)
        d.backward(g.to(d))
    finally:
        lpips.FUSED = old
    return d.detach(), p.grad


@pytest.mark.gpu
def test_perceptual_loss_module_uses_the_kernel():
    """lpips.PerceptualLoss, channels_last on the GPU, against the same module in float64 on the CPU: distances and the
    gradient of the image, under the gate with FUSED off as the fp32 term; five forward and five backward launches.
    m(b, b) is exactly 0: the module computes the features of one tensor once.  (Two passes of the MIOpen trunk over equal
    values are not bit-identical on the MI355X; m(b, copy of b) measured 3.5e-15 to 3.8e-15 with the kernel and with the
    composite alike, against distances of order 1.)"""
    m = _perceptual()
    pred = synth.tensor('lpd/mod/pred', (2, 3, 64, 64), dist='uniform')
    target = synth.tensor('lpd/mod/target', (2, 3, 64, 64), dist='uniform')
    g = upstream(2)
    ref = _module_run(copy.deepcopy(m).double(), pred.double(), target.double(), g.double(), False)
    mg = m.to(dev()).to(memory_format=torch.channels_last)
    pg, tg = nhwc(pred), nhwc(target)
    (on, obs) = observed(lambda: _module_run(mg, pg, tg, g.to(dev()), True))
    (off, obs_off) = observed(lambda: _module_run(mg, pg, tg, g.to(dev()), False))
    assert obs_off == []
    hw = [64 * 64, 32 * 32, 16 * 16, 8 * 8, 4 * 4]
    fwd = [(2, c, p, 0) for c, p in zip((64, 128, 256, 512, 512), hw)]
    assert obs[:5] == fwd and sorted(obs[5:]) == sorted((n, c, p, 1) for n, c, p, _ in fwd)
    gate('PerceptualLoss d', err(on[0], ref[0]), err(off[0], ref[0]))
    gate('PerceptualLoss d/d image', err(on[1], ref[1]), err(off[1], ref[1]))
    import lpips
    assert lpips.FUSED
    with torch.no_grad():
        assert torch.count_nonzero(mg(tg, tg)) == 0                                       # m(b, b) = 0 exactly
        # a copy of b goes through the trunk a second time, and MIOpen's convolutions differ in the last bit from call to
        # call (measured: tap 1 differs by 1.2e-7 between two passes over the same values), with the composite as well
        again = mg(tg, tg.clone())
        print(f'm(b, copy of b) = {again.flatten().tolist()} (d(b, other image) = {on[0].flatten().tolist()})')
        assert float(again.abs().max()) <= 1e-10 * float(on[0].abs().max())
    mg.train()                                                                            # dropout active: the composite
    try:
        _, obs_train = observed(lambda: mg(pg, tg))
    finally:
        mg.eval()
    assert obs_train == []


def _rel_diffs(a, b):
    return sorted(float((a[k] - b[k]).abs().max()) / float(b[k].abs().max()) for k in a if float(b[k].abs().max()) > 0)


@pytest.mark.gpu
def test_g_step_agrees_with_the_composite():
    """One G_Loss_BackProp with lpips_model on the 64^2 training-step networks, FUSED on and off.

    The weighted LPIPS term agrees to 1e-5 relative (measured: bit-equal).

    The parameter gradients were to agree to 1e-5 of each tensor's max.  They cannot: the step itself is not reproducible
    to that level on the MI355X.  Two runs of the unchanged composite step differ by max|diff| / max|grad| of 5.0e-3 to
    1.2e-2 at the worst tensor (e_wp.styles.3.convs.0.weight, e_wp.styles.9.convs.0.weight) and 7.0e-6 to 6.1e-5 at the
    median tensor of 394, and two runs without any LPIPS term by 2.7e-3 / 1.2e-5: MIOpen's convolutions differ in the last
    bit from call to call and the encoders' PReLU / LeakyReLU kinks amplify that (tests/test_hip_train.py, confirm_kinks).
    Fused against composite measured 5.1e-3 to 1.2e-2 worst / 3.5e-6 to 6.1e-5 median (6.06e-5 in the run whose composite
    pair gave 6.07e-5), fused against fused 5.0e-3 / 5.3e-6.  A flipped kink is a discrete event, so the
    worst tensor jumps between 5e-3 and 1.2e-2 from one pair of runs to the next, whichever forms are compared, and the
    median tensor sits near 5e-6 for some pairs of runs and near 6e-5 for others.  If the fused step is one more draw from
    the composite step's own distribution, it is as near to some composite run as the composite runs are to each other.
    Hence, with three composite runs:

        median tensor: min over composite runs of diff(fused, composite)
                           <= 2 * max over pairs of diff(composite, composite) + 1e-5
                       (the gate used for the kernels, with the composite step's own run-to-run spread as the reference
                       error)
        worst tensor:  min over composite runs of diff(fused, composite) <= KINK_MAX of tests/test_hip_train.py
                       (0.1: what one flipped kink may move a tensor by, the suite's allowance against the golden gradients)

    The sharp statement about the fused term is test_perceptual_loss_module_uses_the_kernel (the image gradient, 1e-7)."""
    import cases
    import lpips
    import test_hip_train as H
    import train_3_encoder as T
    nets = H.build_nets(cases.TRAIN_STEP_CASE['size'], with_d=True, n_mlp=2)
    photo, render, ref, _ = H.train_inputs()
    args = H.train_args()
    lp = _perceptual().to(dev()).to(memory_format=torch.channels_last)
    G = PinNoise(nets['g'])
    trained = [(k, n) for k in ('g', 'e_tsr', 'e_w', 'e_wp') for n in nets[k].named_parameters()]

    def step(fused):
        old = lpips.FUSED
        lpips.FUSED = fused
        try:
            ld = {}
            (_, obs) = observed(lambda: T.G_Loss_BackProp(G, nets['e_tsr'], nets['e_w'], nets['e_wp'], nets['d'], photo,
                                                          render, ref, args, ld, None, lpips_model=lp))
        finally:
            lpips.FUSED = old
        grads = {f'{k}.{name}': p.grad.detach().clone() for k, (name, p) in trained if p.grad is not None}
        return float(ld['lpips'].detach()), grads, len(obs)

    step(False)                                  # the first call of each convolution picks its kernel: not compared
    offs = [step(False) for _ in range(3)]
    l_on, g_on, n_on = step(True)
    l_off = offs[0][0]
    assert ([o[2] for o in offs], n_on) == ([0, 0, 0], 10)
    print(f'lpips term: fused {l_on!r} composite {[o[0] for o in offs]!r} rel {abs(l_on - l_off) / abs(l_off):.3e}')
    assert abs(l_on - l_off) <= 1e-5 * abs(l_off)
    assert all(g_on.keys() == o[1].keys() for o in offs) and len(g_on) > 20
    fused = [_rel_diffs(g_on, o[1]) for o in offs]
    spread = [_rel_diffs(offs[i][1], offs[j][1]) for i, j in ((0, 1), (0, 2), (1, 2))]
    mid = len(fused[0]) // 2
    for what, pick in (('worst tensor', -1), ('median tensor', mid)):
        print(f'parameter gradients, {what}: fused vs composite {[f"{d[pick]:.3e}" for d in fused]}, '
              f'composite vs composite {[f"{d[pick]:.3e}" for d in spread]}')
    assert min(d[mid] for d in fused) <= 2 * max(d[mid] for d in spread) + 1e-5
    assert min(d[-1] for d in fused) <= H.KINK_MAX
