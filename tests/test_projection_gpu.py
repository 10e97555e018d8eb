"""GPU tests of the image projection: the two kernels of the criterion's image stage (csrc/projection_loss.hip) against
the header's formula bit for bit, against the aten composite and its float64 autograd, the criterion in the fused and the
composite form against the reference's values (tests/golden/projection.npz), and the Generator trajectories of
tests/projection_cases.py through Evaluation.image_projection.

Gates: 4 x the reference's (or the fp32 composite's) own error against float64 plus the project's 2e-6 relative floor
(DESIGN section 0), unless a test says otherwise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import launches
import nets
import projection_cases as pj
import synth
from gpumem import dev, guarded, guards_intact
from nets import load, scaling

pytestmark = pytest.mark.gpu

FLOOR = 2e-6
K = 0.37            # the backward's coefficient in the kernel tests


_inputs = {}


def kernel_inputs(batch, size):
    """(x, target, mask, g_y) on the device, computed once per shape and never written: x is 1.3 * U(-1, 1) (a quarter
    beyond the clamp) with exact +-1 sprinkled in, the mask has zeros, g_y is N(0, 1) in channels_last storage."""
    key = (batch, size)
    if key not in _inputs:
        shape = (batch, 3, size, size)
        x = 1.3 * synth.tensor(f'projection/kernel/x/{batch}x{size}', shape, dist='uniform')
        flat = x.view(-1)
        flat[1::101] = 1.0
        flat[2::103] = -1.0
        t = synth.tensor(f'projection/kernel/t/{batch}x{size}', shape, dist='uniform')
        m = (synth.tensor(f'projection/kernel/mask/{size}', (size, size), dist='uniform') + 1) / 2
        m = torch.where(m < 0.25, torch.zeros_like(m), m)
        g = synth.tensor(f'projection/kernel/gy/{batch}', (batch, 3, 256, 256))
        _inputs[key] = (x.to(dev()), t.to(dev()), m.to(dev()),
                        g.to(dev()).contiguous(memory_format=torch.channels_last))
    return _inputs[key]


def reduced(a, f):
    """The header's reduction of an already clamped image in fp32 torch ops, in the header's association."""
    if f == 1:
        return a
    o = f // 2 - 1
    p, q = a[:, :, o::f, o::f], a[:, :, o::f, o + 1::f]
    r, s = a[:, :, o + 1::f, o::f], a[:, :, o + 1::f, o + 1::f]
    return 0.5 * (0.5 * p + 0.5 * q) + 0.5 * (0.5 * r + 0.5 * s)


def expected_y(x, shift, scale, f):
    """(v - shift) in fp32, then the float64 quotient rounded to fp32 (= the correctly rounded fp32 quotient)."""
    u = reduced(torch.clamp(x, -1., 1.), f) - shift.view(1, 3, 1, 1)
    assert u.dtype == torch.float32
    return (u.double() / scale.view(1, 3, 1, 1).double()).float()


def tap_weight(size, f):
    """w_f as an [S, S] tensor: 1 at f = 1, 1/4 at f = 2, 1/4 on rows and columns 4i+1, 4i+2 at f = 4 and 0 elsewhere."""
    if f == 1:
        return torch.ones(size, size, device=dev())
    if f == 2:
        return torch.full((size, size), 0.25, device=dev())
    on = torch.zeros(size, device=dev())
    on[1::4] = 1
    on[2::4] = 1
    return 0.25 * on[:, None] * on[None, :]


SHAPES = [(b, s) for s in (256, 512, 1024) for b in (1, 3)]


@pytest.mark.parametrize('batch,size', SHAPES, ids=[f'{b}x{s}' for b, s in SHAPES])
def test_forward_kernel(batch, size):
    """With and without mask, with and without y, through the raw entry point into NaN-filled buffers between guard words:
    every output element is written, no guard word changes; y is the header's formula bit for bit and within one ulp of
    clamp -> F.interpolate -> ScalingLayer; the partials' float64 sum is within 1e-6 of the float64 sum of the fp32
    squares; a second run gives the same partial bits; the binding returns the same tensors."""
    from op import _native
    L = _native.lib()
    x, t, mask, _ = kernel_inputs(batch, size)
    f = size // 256
    sl = scaling()
    shift, scale = sl.shift.reshape(3), sl.scale.reshape(3)
    assert L.fmgan_projection_loss_select(batch, size, size, f) == f
    blocks = L.fmgan_projection_loss_blocks(batch, size, size, f)
    want_y = expected_y(x, shift, scale, f)
    comp_y = sl(F.interpolate(torch.clamp(x, -1., 1.), size=256, mode='bilinear', align_corners=False))
    stream = torch.cuda.current_stream().cuda_stream
    for m in (None, mask):
        sq = (x - t) ** 2 if m is None else (x - t) ** 2 * m
        want_sum = float(sq.double().sum())
        for with_y in (True, False):
            pbuf, partial = guarded((blocks,))
            ybuf, y = guarded((batch, 256, 256, 3))
            runs = []
            for _ in range(2):
                st = L.fmgan_projection_loss_fwd_f32(_native.fp(x), _native.fp(t), _native.fp(m), _native.fp(shift),
                                                     _native.fp(scale), partial.data_ptr(),
                                                     y.data_ptr() if with_y else None, batch, size, size, f, stream)
                assert st == 0, st
                torch.cuda.synchronize()
                runs.append(partial.clone())
            assert guards_intact(pbuf) and guards_intact(ybuf) and bool(torch.isfinite(partial).all())
            assert torch.equal(runs[0], runs[1])
            got_sum = float(partial.sum(dtype=torch.float64))
            rel = abs(got_sum - want_sum) / want_sum
            print(f'{batch}x{size} mask {m is not None} y {with_y}: sq_sum {got_sum:.9e} float64 {want_sum:.9e} rel {rel:.2e}')
            assert rel <= 1e-6
            if with_y:
                assert bool(torch.isfinite(y).all()) and torch.equal(y.permute(0, 3, 1, 2), want_y)
                yy = y.permute(0, 3, 1, 2)
                big = torch.maximum(yy.abs(), comp_y.abs())
                ulp = torch.nextafter(big, torch.full_like(big, float('inf'))) - big
                worst = float(((yy - comp_y).abs() / ulp).max())
                print(f'{batch}x{size}: max |y - composite| in ulps {worst:.2f}, bit-equal {torch.equal(yy, comp_y)}')
                assert worst <= 1.0
            else:
                assert bool(torch.isnan(y).all())
            bound = _native.projection_loss_fwd(x, t, m, sl.shift.reshape(3), sl.scale.reshape(3), with_y)
            assert torch.equal(bound[0], partial)
            if with_y:
                assert tuple(bound[1].shape) == (batch, 3, 256, 256)
                assert bound[1].is_contiguous(memory_format=torch.channels_last)
                assert torch.equal(bound[1], y.permute(0, 3, 1, 2))
            else:
                assert bound[1] is None


def _float64_grad(x, t, m, g_y, sl, dtype):
    """grad_x of K/2 * sq_sum + <y, g_y> by autograd through the composite in `dtype`."""
    from op import projection_loss as PL
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    sl = scaling().to(dtype)
    sq, y = PL.projection_stage_composite(xx, t.to(dtype), None if m is None else m.to(dtype), sl, g_y is not None)
    outs, grads = [sq], [torch.tensor(K / 2, dtype=dtype, device=x.device)]
    if g_y is not None:
        outs.append(y), grads.append(g_y.to(dtype))
    return torch.autograd.grad(outs, [xx], grads)[0]


@pytest.mark.parametrize('batch,size', SHAPES, ids=[f'{b}x{s}' for b, s in SHAPES])
def test_backward_kernel(batch, size):
    """With and without mask, with and without g_y, into a NaN-filled guarded buffer: grad_x is within 4 x the fp32
    composite's own error + 2e-6 of the float64 autograd of the composite, relative to max |grad|; it is exactly the mse
    term (k * (x - t)) * mask where |x| > 1 and, at f = 4, on the rows and columns that carry no tap; at x = +-1 the
    trunk's gradient passes."""
    from op import _native
    L = _native.lib()
    x, t, mask, g_y = kernel_inputs(batch, size)
    f = size // 256
    sl = scaling()
    scale = sl.scale.reshape(3)
    k = torch.tensor([K], dtype=torch.float32, device=dev())
    stream = torch.cuda.current_stream().cuda_stream
    wf = tap_weight(size, f)
    for m in (None, mask):
        mse = k * (x - t) if m is None else (k * (x - t)) * m
        for g in (g_y, None):
            gbuf, grad = guarded((batch, 3, size, size))
            st = L.fmgan_projection_loss_bwd_f32(_native.fp(x), _native.fp(t), _native.fp(m), _native.fp(g),
                                                 _native.fp(k), _native.fp(scale), grad.data_ptr(), batch, size, size, f,
                                                 stream)
            assert st == 0, st
            torch.cuda.synchronize()
            assert guards_intact(gbuf) and bool(torch.isfinite(grad).all())
            g64 = _float64_grad(x, t, m, g, sl, torch.float64)
            g32 = _float64_grad(x, t, m, g, sl, torch.float32)
            top = float(g64.abs().max())
            own = float((g32.double() - g64).abs().max())
            err = float((grad.double() - g64).abs().max())
            print(f'{batch}x{size} mask {m is not None} g_y {g is not None}: max|grad| {top:.3e} kernel err {err:.3e} '
                  f'fp32 composite err {own:.3e} gate {4 * own + FLOOR * top:.3e}')
            assert err <= 4 * own + FLOOR * top
            if g is None:
                assert torch.equal(grad, mse)
                continue
            outside = (x.abs() > 1) | (wf == 0)
            assert bool(outside.any()) and torch.equal(grad[outside], mse[outside])
            term = wf * (F.interpolate(g.contiguous(), scale_factor=f, mode='nearest') / sl.scale) if f > 1 else g / sl.scale
            edge = (x.abs() == 1) & (wf > 0) & (term != 0)
            assert int(edge.sum()) > 100
            passed = (grad - mse)[edge]
            assert bool((passed != 0).all())
            assert float(((passed - term[edge]).abs() / term[edge].abs().clamp_min(1e-3)).max()) <= 1e-4
            bound = _native.projection_loss_bwd(x, t, m, g, k, scale)
            assert torch.equal(bound, grad)


def test_mask_multiplies_so_a_nan_under_a_zero_of_the_mask_leaks():
    """The kernels multiply by the mask, as the reference's weighted_mse_loss does: a NaN of the target where the mask is 0
    makes sq_sum NaN and its own grad_x elements NaN (NaN * 0), and nothing else; the composite does the same.  Callers
    that mask out invalid pixels must make them finite first."""
    from op import projection_loss as PL
    x, t, mask, g_y = kernel_inputs(1, 512)
    t = t.clone()
    hole = (mask == 0)
    assert int(hole.sum()) > 1000
    rows, cols = torch.nonzero(hole, as_tuple=True)
    t[0, 1, rows[:50], cols[:50]] = float('nan')
    sl = scaling()
    for stage in (PL.projection_stage, PL.projection_stage_composite):
        xx = x.clone().requires_grad_(True)
        sq, y = stage(xx, t, mask, sl, True)
        (sq + (y * g_y).sum()).backward()
        bad = torch.isnan(xx.grad)
        assert bool(torch.isnan(sq)) and bool(torch.isfinite(y).all())
        assert int(bad.sum()) == 50 and bool(bad[0, 1, rows[:50], cols[:50]].all())


def test_stage_autograd_and_double_backward():
    """projection_stage under autograd on the kernels: sq_sum is a 0-dim fp32 tensor, bit-identical run to run; the
    gradient of a weighted sum of both outputs is the backward kernel's with k = 2 * weight; an unused y costs nothing
    (grad_y None); a second differentiation raises; a target that wants a gradient is not served."""
    from op import _native, projection_loss as PL
    x, t, mask, g_y = kernel_inputs(3, 512)
    sl = scaling()
    assert PL.projection_stage_serves(x, t, mask, sl) and not PL.projection_stage_serves(x, t.clone().requires_grad_(), mask, sl)
    assert not PL.projection_stage_serves(x[:, :, ::2], t[:, :, ::2], None, sl)
    xx = x.clone().requires_grad_(True)
    sq, y = PL.projection_stage(xx, t, mask, sl, True)
    sq2, _ = PL.projection_stage(xx, t, mask, sl, False)
    assert sq.ndim == 0 and sq.dtype == torch.float32 and torch.equal(sq, sq2) and _ is None
    loss = sq * (K / 2) + (y * g_y).sum()
    grad, = torch.autograd.grad(loss, xx, create_graph=True)
    k = torch.tensor([K], dtype=torch.float32, device=dev())
    want = _native.projection_loss_bwd(x, t, mask, g_y, k, sl.scale.reshape(3))
    assert float((grad - want).abs().max()) <= 1e-6 * float(want.abs().max())      # k = 2 * (K / 2) rounds once
    only_sq, = torch.autograd.grad(sq2 * (K / 2), xx)
    assert torch.equal(only_sq, _native.projection_loss_bwd(x, t, mask, None, k, sl.scale.reshape(3)))
    twice, = torch.autograd.grad(sq ** 2, xx, create_graph=True)      # a gradient that depends on x
    with pytest.raises(RuntimeError, match='once_differentiable'):
        twice.sum().backward()


# ------------------------------------------------------------------------------------------------ the criterion
@pytest.fixture(scope='module')
def percept():
    return nets.percept(dev())


def _stages(rec):
    """(forward, backward) launches of the image stage: the direction is the last item of the launch's info."""
    return tuple(sum(1 for i in rec.infos('projection_loss') if i[-1] == direction) for direction in (0, 1))


SERVED = ['c256_mse', 'c256_mse_mask', 'c256_lpips', 'c256_mix', 'c512_mse_mask', 'c512_lpips']


def _criterion_gates(c, g, i):
    """(loss gate, gradient gate) of call i.  Loss: 4 x |loss32 - loss64| + 2e-6 |loss64| of that call.  Gradient: 4 x the
    reference's own max |grad32 - grad64| + 2e-6 max |grad64|, the reference's error taken as the largest over the case's
    calls in which LPIPS was in the same state as in call i (as test_ppl_gpu takes the largest over a case's pairs): the
    VGG trunk is piecewise linear, an fp32 evaluation lands on the other side of a ReLU or max-pool kink in some calls and
    not in others (the reference's own figure ranges from 2e-6 to 3e-2 of max |grad| over the LPIPS calls of the
    fixture), and on which calls it does differs between the CPU and MIOpen."""
    k = f"{c['name']}/{i}/"
    l64 = float(g[k + 'loss64'])
    same = [j for j in range(len(c['amplitudes'])) if bool(g[f"{c['name']}/{j}/use_lpips"]) == bool(g[k + 'use_lpips'])]
    own = max(float(g[f"{c['name']}/{j}/grad_err"]) for j in same)
    return 4 * abs(float(g[k + 'loss']) - l64) + FLOOR * abs(l64), 4 * own + FLOOR * float(g[k + 'grad_max64'])


@pytest.mark.parametrize('name', SERVED)
def test_criterion_cases_fused_and_composite(name, golden, percept, monkeypatch):
    """The fixture cases the kernels serve, call by call in the fused and in the composite form: each against the
    reference's float64 run under _criterion_gates, and the two against each other: under the same gates where LPIPS is
    on (two fp32 evaluations that both lie within the gate of the float64 value may differ by that much from each other;
    MIOpen's trunk is not reproducible call to call either), and within 2e-6 of the loss and 4 ulp of max |grad| where it
    is off (no trunk: both forms are deterministic); LPIPS on exactly where the reference had it on; fused, every call is one forward and one
    backward stage launch, unfused none."""
    from Evaluation.image_projection import project
    c = pj.CRITERION_BY_NAME[name]
    g = golden('projection')
    s = c['stride']
    results = {}
    for fuse in (True, False):
        monkeypatch.setattr(project, 'PROJECT_FUSE', fuse)
        crit = project.ImageReconstructionLoss(device=dev(), loss=c['loss'],
                                               percept=percept if c['loss'] != 'mse' else None)
        for i in range(len(c['amplitudes'])):
            k = f'{name}/{i}/'
            output, target, mask = (None if v is None else v.to(dev()) for v in pj.criterion_inputs(c, i))
            output.requires_grad_(True)
            with launches.observed() as rec:
                loss = crit(output, {'target': target, 'mask': mask})
                loss.backward()
            assert _stages(rec) == ((1, 1) if fuse else (0, 0))
            assert crit.use_lpips == bool(g[k + 'use_lpips'])
            gate, ggate = _criterion_gates(c, g, i)
            err = abs(float(loss.detach()) - float(g[k + 'loss64']))
            gerr = float(np.abs(output.grad[:, :, ::s, ::s].double().cpu().numpy() - g[k + 'grad64']).max())
            print(f'{k} {"fused" if fuse else "composite"} loss {float(loss.detach()):.9e} loss64 '
                  f'{float(g[k + "loss64"]):.9e} err {err:.3e} gate {gate:.3e}; grad err {gerr:.3e} gate {ggate:.3e} (max '
                  f'{float(g[k + "grad_max64"]):.3e})')
            assert err <= gate and gerr <= ggate
            results[fuse, i] = (float(loss.detach()), output.grad)
    for i in range(len(c['amplitudes'])):
        gate, ggate = _criterion_gates(c, g, i)
        if not bool(g[f'{name}/{i}/use_lpips']):
            # no trunk in the call: both forms are deterministic fp32 evaluations of the same expression.  The loss is
            # an fp32 sum of up to 2^20 terms in aten's pairwise order against the kernel's partials added in float64:
            # the project's 2e-6 relative floor; a gradient element is k * (x - t) * mask with k = 2 * mse_weight /
            # denominator rounded in either order: 4 ulp of max |grad|.
            gate = FLOOR * abs(results[False, i][0])
            ggate = 4 * 2.0 ** -23 * float(results[False, i][1].abs().max())
        dl = abs(results[True, i][0] - results[False, i][0])
        dg = float((results[True, i][1] - results[False, i][1]).abs().max())
        print(f'{name}/{i}/ fused against composite: loss {dl:.3e} gate {gate:.3e}; grad {dg:.3e} gate {ggate:.3e}')
        assert dl <= gate and dg <= ggate


# ------------------------------------------------------------------------------------------------ trajectories
_generators = {}


def _generator(size):
    import stylegan2
    if size not in _generators:
        _generators[size] = load(stylegan2.Generator(size, pj.LATENT_DIM, 2, channel_multiplier=1), 'generator', 4)
        _generators[size].requires_grad_(False)
    return _generators[size]


# Floor of the displacement gate: twice the largest relative L2 difference between two HIP runs of the same case
# (MIOpen's trunk is not reproducible call to call), measured on the MI355X by tools/bench_projection.py, part (c)
# (profiles/projection.md), in three runs of the tool: g64_w 1.21e-3 / 6.2e-4 / 2.05e-3, g64_wplus 7.8e-4 / 9.1e-4 /
# 9.9e-4, g256_w 4.5e-4 / 1.93e-3 / 1.57e-3 (the widest noise maps each time)  ->  2 * 2.05e-3.
DISPLACEMENT_FLOOR = 4.09e-3


@pytest.mark.parametrize('name', ['g64_w', 'g64_wplus', 'g256_w'])
def test_generator_trajectories(name, golden, percept):
    """optimize + ImageReconstructionLoss('mse+lpips') + Adam on the narrow Generator, set up as Image_Projector does from
    fixed samples.  Per step the loss against the reference's float64 run (4 x |loss32 - loss64| + 2e-6 |loss64|); the
    relative L2 error of the total displacement of W and of every noise map against the float64 fixture (4 x the
    reference's own fp32 figure + DISPLACEMENT_FLOOR = 4.09e-3, twice the largest
    difference measured between two HIP runs of one case: 2.05e-3).  The target goes through the trunk once; g256_w runs the fused
    stage once per step and direction, g64 (upsampled) the composite."""
    from test_projection import _run_trajectory
    c = pj.TRAJECTORY_BY_NAME[name]
    g = golden('projection')
    gen = _generator(c['size'])
    trunk = []
    hook = percept.net.net.register_forward_hook(lambda m, i, o: trunk.append(1))
    try:
        with launches.observed() as rec:
            history, last, disp, crit = _run_trajectory(c, gen, percept, device=dev())
    finally:
        hook.remove()
    steps = c['iterations'] + 1
    assert len(trunk) == steps + 1
    assert _stages(rec) == ((steps, steps) if c['size'] == 256 else (0, 0))
    losses = np.array([float(l) for _, l in history])
    l32, l64 = g[name + '/loss'], g[name + '/loss64']
    gate = 4 * np.abs(l32 - l64) + FLOOR * np.abs(l64)
    for i in range(steps):
        print(f'{name} step {i}: loss {losses[i]:.9e} loss64 {l64[i]:.9e} err {abs(losses[i] - l64[i]):.3e} gate {gate[i]:.3e}')
    want = [g[name + '/dW64']] + [g[f'{name}/dnoise{i}64'] for i in range(len(disp) - 1)]
    ref_err = [float(g[name + '/dW_err'])] + list(g[name + '/dnoise_err'])
    errs = []
    for j, (d, w, e) in enumerate(zip(disp, want, ref_err)):
        errs.append(np.linalg.norm(pj.noise_sample(d).numpy() - w) / np.linalg.norm(w))
        print(f'{name} displacement {"W" if j == 0 else "noise%d" % (j - 1)}: rel L2 {errs[-1]:.3e} reference {e:.3e} '
              f'gate {4 * e + DISPLACEMENT_FLOOR:.3e}')
    assert np.all(np.abs(losses - l64) <= gate)
    assert all(err <= 4 * e + DISPLACEMENT_FLOOR for err, e in zip(errs, ref_err))


def test_image_projector_on_the_generator():
    """Image_Projector with the narrow Generator(64) in W+ from a float tensor, and in W from a list of PIL images (the
    GPU form of ToTensor + Normalize, Util.image_io): two CPU tensors of the target's shape, the Generator's parameters
    and buffers bit-unchanged."""
    from PIL import Image
    from Evaluation.image_projection import image_projector as IP, project
    gen = _generator(64)
    before = {k: v.clone() for k, v in gen.state_dict().items()}
    target = pj.trajectory_start(pj.TRAJECTORY_BY_NAME['g64_wplus'], gen, device=dev())[2]
    u8 = ((target.permute(0, 2, 3, 1) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
    images = [Image.fromarray(a) for a in u8]
    t = IP.img_transform(images, dev())
    assert t.is_cuda and torch.equal(t.cpu(), IP.img_transform(images, 'cpu'))
    for per_layer, tgt in ((True, target), (False, images)):
        inp, out = IP.Image_Projector(gen, dev(), per_layer, tgt, 'Adam', num_iters=3, print_iters=0,
                                      criterion=project.ImageReconstructionLoss(device=dev(), loss='mse'))
        assert tuple(inp.shape) == tuple(out.shape) == (2, 3, 64, 64) and inp.device.type == out.device.type == 'cpu'
        assert bool(torch.isfinite(out).all()) and not torch.equal(inp, out)
    assert all(torch.equal(v, before[k]) for k, v in gen.state_dict().items())
