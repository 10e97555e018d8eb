"""CPU tests of the image projection (Evaluation/image_projection), the host logic of its criterion's image stage
(op/projection_loss.py, fmgan_projection_loss_select) and lpips' cached-target methods: everything here runs without a
device.  The kernels and the Generator trajectories are in tests/test_projection_gpu.py.

Gates against tests/golden/projection.npz follow the project's standing rule for an fp32 path against the reference's
float64 run: 4 x the reference's own fp32-vs-float64 error plus a 2e-6 relative floor."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nets
import projection_cases as pj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED, EOVERFLOW = 0, -1, -2, -4
FLOOR = 2e-6


@pytest.fixture(scope='module')
def percept():
    return nets.percept()


# ------------------------------------------------------------------------------------------------ library and binding
def test_library_exports_the_projection_entry_points():
    """The four symbols are exported, declared in the header, and bound in op/_native/core.py's table with the header's
    argument kinds in the header's order."""
    hdr = open(os.path.join(ROOT, 'include', 'fmgan_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    L = nets.lib()
    for name in ('fmgan_projection_loss_select', 'fmgan_projection_loss_blocks', 'fmgan_projection_loss_fwd_f32',
                 'fmgan_projection_loss_bwd_f32'):
        params = re.search(r'\b' + name + r'\s*\(([^()]*)\)\s*;', hdr).group(1).split(',')
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for p, t in zip(params, fn.argtypes):
            assert t is (ctypes.c_void_p if '*' in p else ctypes.c_int), (name, p)
        assert fn.restype is ctypes.c_int
    assert len(L.fmgan_projection_loss_fwd_f32.argtypes) == 12 and len(L.fmgan_projection_loss_bwd_f32.argtypes) == 12


def test_select_returns_the_plan_or_the_launch_status():
    """fmgan_projection_loss_select is the launches' plan with the launch left out: f for S = 256 f, f in {1, 2, 4}, and
    for each refused argument class the status both launches return (refused before any HIP call: the pointers are
    placeholders).  fmgan_projection_loss_blocks is 128 per sample where served and 0 elsewhere."""
    L = nets.lib()
    fake = ctypes.c_void_p(0x1000)
    for batch in (1, 3, 8):
        for f in (1, 2, 4):
            assert L.fmgan_projection_loss_select(batch, 256 * f, 256 * f, f) == f
            assert L.fmgan_projection_loss_blocks(batch, 256 * f, 256 * f, f) == 128 * batch
    refused = {
        EINVAL: [(0, 256, 256, 1), (-1, 256, 256, 1), (1, 0, 256, 1), (1, 256, -4, 1), (1, 256, 256, 0),
                 (1, 256, 256, -1), (-1, 64, 64, 1)],
        EUNSUPPORTED: [(1, 64, 64, 1), (1, 768, 768, 3), (1, 768, 768, 2), (1, 512, 256, 2), (1, 256, 512, 1),
                       (1, 512, 512, 1), (1, 1024, 1024, 2), (1, 2048, 2048, 8), (1, 256, 256, 3)],
        EOVERFLOW: [(1 << 24, 256, 256, 1), (0x7fffffff, 1024, 1024, 4)],
    }
    for status, rows in refused.items():
        for args in rows:
            assert L.fmgan_projection_loss_select(*args) == status, (status, args)
            assert L.fmgan_projection_loss_blocks(*args) == 0, args
            assert L.fmgan_projection_loss_fwd_f32(*[fake] * 7, *args, None) == status, (status, args)
            assert L.fmgan_projection_loss_bwd_f32(*[fake] * 7, *args, None) == status, (status, args)
    assert L.fmgan_projection_loss_select((1 << 24) - 1, 256, 256, 1) == 1


def test_null_pointers_are_einval_before_the_plan():
    """x, target, partial (forward) and x, target, k, grad_x (backward) must be there; y needs shift and scale, g_y needs
    scale; mask, y and g_y may be NULL.  The shape is one the library declines, so nothing is ever launched: a NULL
    among the required pointers still gives FMGAN_EINVAL, everything else the plan's FMGAN_EUNSUPPORTED."""
    L = nets.lib()
    fake = ctypes.c_void_p(0x1000)
    shape = (1, 64, 64, 1)
    # forward: x, target, mask, shift, scale, partial, y
    for k, want in ((0, EINVAL), (1, EINVAL), (2, EUNSUPPORTED), (3, EINVAL), (4, EINVAL), (5, EINVAL), (6, EUNSUPPORTED)):
        ptrs = [fake] * 7
        ptrs[k] = None
        assert L.fmgan_projection_loss_fwd_f32(*ptrs, *shape, None) == want, k
    assert L.fmgan_projection_loss_fwd_f32(fake, fake, None, None, None, fake, None, *shape, None) == EUNSUPPORTED
    # backward: x, target, mask, g_y, k, scale, grad_x
    for k, want in ((0, EINVAL), (1, EINVAL), (2, EUNSUPPORTED), (3, EUNSUPPORTED), (4, EINVAL), (5, EINVAL), (6, EINVAL)):
        ptrs = [fake] * 7
        ptrs[k] = None
        assert L.fmgan_projection_loss_bwd_f32(*ptrs, *shape, None) == want, k
    assert L.fmgan_projection_loss_bwd_f32(fake, fake, None, None, fake, None, fake, *shape, None) == EUNSUPPORTED


def test_stage_serves_nothing_on_the_cpu_and_the_binding_refuses_cpu_tensors():
    from op import _native, projection_loss as PL
    x = torch.zeros(1, 3, 256, 256)
    assert not PL.projection_stage_serves(x, x)
    with pytest.raises(RuntimeError):
        _native.projection_loss_fwd(x, x, None, torch.zeros(3), torch.ones(3))
    with pytest.raises(ValueError):
        _native.projection_loss_fwd(x, x[:, :, :128], None, torch.zeros(3), torch.ones(3))


# ------------------------------------------------------------------------------------------------ the stage
def _fake_kernels(monkeypatch):
    """The two binding calls answered by aten on the CPU, so that the autograd Function can run here."""
    from op import _native, projection_loss as PL

    def fwd(x, target, mask, shift, scale, want_y=True):
        sq = (x - target) ** 2 * (1 if mask is None else mask)
        y = (PL.projection_resize(x) - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1) if want_y else None
        return sq.sum().reshape(1), y

    def bwd(x, target, mask, g_y, k, scale):
        with torch.enable_grad():
            xx = x.detach().requires_grad_(True)
            sq, y = fwd(xx, target, mask, torch.zeros(3), scale, g_y is not None)
            outs, grads = [sq], [k / 2]
            if g_y is not None:
                outs.append(y), grads.append(g_y)
            return torch.autograd.grad(outs, [xx], grads)[0]
    monkeypatch.setattr(_native, 'projection_loss_fwd', fwd)
    monkeypatch.setattr(_native, 'projection_loss_bwd', bwd)


def test_stage_function_matches_the_composite_and_refuses_a_double_backward(monkeypatch):
    """ProjectionStageFunction with the binding answered by aten: value and gradient are the composite's, the upstream
    gradient of sq_sum reaches the backward as the device scalar k = 2 * grad, and differentiating the gradient again
    raises (once_differentiable)."""
    import lpips
    from op import projection_loss as PL
    _fake_kernels(monkeypatch)
    sl = lpips.ScalingLayer()
    c = pj.CRITERION_BY_NAME['c64_mse_mask']
    x, t, mask = pj.criterion_inputs(c, 0)
    x = torch.nn.functional.interpolate(x, size=256)[:1]
    t = torch.nn.functional.interpolate(t, size=256)[:1]
    mask = torch.nn.functional.interpolate(mask[None, None], size=256)[0, 0]
    probe = torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(1))
    grads = []
    for form in ('function', 'composite'):
        xx = x.clone().requires_grad_(True)
        if form == 'function':
            sq, y = PL.ProjectionStageFunction.apply(xx, t, mask, sl.shift.reshape(3), sl.scale.reshape(3), True)
        else:
            sq, y = PL.projection_stage_composite(xx, t, mask, sl)
        loss = 0.37 * sq + (y * probe).sum()
        g, = torch.autograd.grad(loss, xx, create_graph=True)
        grads.append((float(loss.detach()), g))
    assert abs(grads[0][0] - grads[1][0]) <= 1e-5 * abs(grads[1][0])
    assert float((grads[0][1] - grads[1][1]).detach().abs().max()) <= 1e-5 * float(grads[1][1].detach().abs().max())
    for form in ('composite', 'function'):                          # a gradient that depends on x, differentiated again
        xx = x.clone().requires_grad_(True)
        if form == 'function':
            sq, _ = PL.ProjectionStageFunction.apply(xx, t, mask, sl.shift.reshape(3), sl.scale.reshape(3), False)
        else:
            sq, _ = PL.projection_stage_composite(xx, t, mask, sl, False)
        g, = torch.autograd.grad(sq ** 2, xx, create_graph=True)
        if form == 'composite':
            g.sum().backward()
            assert xx.grad is not None
        else:
            with pytest.raises(RuntimeError, match='once_differentiable'):
                g.sum().backward()


# ------------------------------------------------------------------------------------------------ the criterion
def _criterion(loss, percept, dtype=torch.float32):
    from Evaluation.image_projection import project
    return project.ImageReconstructionLoss(device='cpu', loss=loss, percept=percept if loss != 'mse' else None).to(dtype)


def test_loss_types_carry_the_references_thresholds(percept):
    from Evaluation.image_projection import project
    assert [_criterion(k, percept).mse_T for k in ('mse', 'mse+lpips+mix', 'mse+lpips')] == [0.0, 0.01, 100]
    assert _criterion('mse', percept).perceptual is None and _criterion('mse+lpips', percept).perceptual is percept
    with pytest.raises(NotImplementedError):
        project.ImageReconstructionLoss(device='cpu', loss='lpips')


@pytest.mark.parametrize('name', [c['name'] for c in pj.CRITERION_CASES])
def test_criterion_reproduces_the_reference(name, golden, percept):
    """Every call of every criterion case on the CPU (the composite stage): the loss within 4 x |loss32 - loss64| +
    2e-6 |loss64| of the reference's float64 value, the gradient with respect to `output` within 4 x grad_err + 2e-6
    grad_max64 at every sampled element, LPIPS on exactly where the reference had it on."""
    c = pj.CRITERION_BY_NAME[name]
    g = golden('projection')
    crit = _criterion(c['loss'], percept)
    for i in range(len(c['amplitudes'])):
        k = f'{name}/{i}/'
        output, target, mask = pj.criterion_inputs(c, i)
        output.requires_grad_(True)
        loss = crit(output, {'target': target, 'mask': mask})
        loss.backward()
        assert crit.use_lpips == bool(g[k + 'use_lpips'])
        l64, gate = float(g[k + 'loss64']), 4 * abs(float(g[k + 'loss']) - float(g[k + 'loss64']))
        gate += FLOOR * abs(l64)
        err = abs(float(loss.detach()) - l64)
        s = c['stride']
        gerr = float(np.abs(output.grad[:, :, ::s, ::s].double().numpy() - g[k + 'grad64']).max())
        ggate = 4 * float(g[k + 'grad_err']) + FLOOR * float(g[k + 'grad_max64'])
        print(f'{k} loss {float(loss.detach()):.9e} loss64 {l64:.9e} err {err:.3e} gate {gate:.3e}; grad err {gerr:.3e} gate '
              f'{ggate:.3e} (max {float(g[k + "grad_max64"]):.3e})')
        assert err <= gate and gerr <= ggate


@pytest.mark.parametrize('name', [c['name'] for c in pj.CRITERION_CASES])
def test_stage_composite_reproduces_the_reference(name, golden, percept):
    """projection_stage_composite itself (the criterion's fall-through and the oracle of the GPU kernel tests) against
    every call of every criterion fixture, the upsampled 64^2 cases included: the loss is built here from its two
    outputs (sq_sum / denominator, plus forward_scaled of y against the scaled target where the reference had LPIPS
    on) and gated, with its gradient with respect to `output`, as in the criterion test above."""
    from op import projection_loss as PL
    c = pj.CRITERION_BY_NAME[name]
    g = golden('projection')
    sl = percept.net.scaling_layer
    for i in range(len(c['amplitudes'])):
        k = f'{name}/{i}/'
        output, target, mask = pj.criterion_inputs(c, i)
        output.requires_grad_(True)
        on = bool(g[k + 'use_lpips'])
        sq, y = PL.projection_stage_composite(output, target, mask, sl, want_y=on)
        assert (y is not None) == on and (y is None or tuple(y.shape) == (c['batch'], 3, 256, 256))
        loss = sq / (output.numel() if mask is None else mask.sum())
        if on:
            with torch.no_grad():
                target_s = PL.projection_trunk_input(target, sl)
            loss = loss + percept.forward_scaled(y, target_s).sum()
        loss.backward()
        l64 = float(g[k + 'loss64'])
        gate = 4 * abs(float(g[k + 'loss']) - l64) + FLOOR * abs(l64)
        err = abs(float(loss.detach()) - l64)
        s = c['stride']
        gerr = float(np.abs(output.grad[:, :, ::s, ::s].double().numpy() - g[k + 'grad64']).max())
        ggate = 4 * float(g[k + 'grad_err']) + FLOOR * float(g[k + 'grad_max64'])
        print(f'{k} composite loss err {err:.3e} gate {gate:.3e}; grad err {gerr:.3e} gate {ggate:.3e}')
        assert err <= gate and gerr <= ggate


def test_threshold_joins_once_and_stays_and_stops_comparing():
    """'mse+lpips+mix' with a stand-in perceptual term: LPIPS is off while mse * mse_weight >= 0.01, joins in the call
    that falls below, stays on when the mse rises again; mse_weight takes part in the comparison; 'mse' never joins; a
    mask together with LPIPS raises and says why."""
    from Evaluation.image_projection import project
    calls = []

    def standin(pred, target):
        calls.append(tuple(pred.shape))
        return ((pred - target) ** 2).mean([1, 2, 3])
    target = torch.zeros(2, 3, 8, 8)
    crit = project.ImageReconstructionLoss(device='cpu', loss='mse+lpips+mix', percept=standin)
    far, near = target + 0.5, target + 0.05
    kw = dict(perceptual_size=16)
    assert float(crit(far, {'target': target, 'mask': None}, **kw)) == pytest.approx(0.25) and not crit.use_lpips
    assert float(crit(near, {'target': target, 'mask': None}, mse_weight=8, **kw)) == pytest.approx(0.02) and not calls
    assert float(crit(near, {'target': target, 'mask': None}, **kw)) == pytest.approx(0.0025 + 2 * 0.0025)
    assert crit.use_lpips and calls == [(2, 3, 16, 16)]
    assert float(crit(far, {'target': target, 'mask': None}, **kw)) == pytest.approx(0.25 + 2 * 0.25) and crit.use_lpips
    assert len(calls) == 2
    never = project.ImageReconstructionLoss(device='cpu', loss='mse')
    assert float(never(near, {'target': target, 'mask': None})) == pytest.approx(0.0025) and not never.use_lpips
    masked = project.ImageReconstructionLoss(device='cpu', loss='mse+lpips', percept=standin)
    with pytest.raises(RuntimeError, match='normalize'):
        masked(near, {'target': target, 'mask': torch.ones(8, 8)})


def test_weighted_mse_divides_by_the_mask_sum_and_caches_it():
    from Evaluation.image_projection import project
    target = torch.zeros(1, 3, 4, 4)
    mask = torch.zeros(4, 4)
    mask[:2] = 1
    crit = project.ImageReconstructionLoss(device='cpu', loss='mse')
    assert float(crit(target + 1, {'target': target, 'mask': mask})) == pytest.approx(3.0)      # 24 / 8
    assert float(crit(target + 1, {'target': target, 'mask': torch.ones(4, 4)})) == pytest.approx(6.0)   # the cached 8
    fresh = project.ImageReconstructionLoss(device='cpu', loss='mse', pre_cache=False)
    fresh(target + 1, {'target': target, 'mask': mask})
    assert float(fresh(target + 1, {'target': target, 'mask': torch.ones(4, 4)})) == pytest.approx(3.0)


def test_cached_target_features_give_forward_scaled(percept):
    """lpips: forward_cached(pred_s, target_features(target_s)) is forward_scaled(pred_s, target_s) on the CPU, bit for
    bit (the same operations in the same order), and forward is untouched."""
    a = pj.criterion_inputs(pj.CRITERION_BY_NAME['c64_lpips'], 0)[0][:, :, :32, :32]
    b = a.flip(3)
    sl = percept.net.scaling_layer
    with torch.no_grad():
        want = percept.forward_scaled(sl(a), sl(b))
        feats = percept.target_features(sl(b))
        got = percept.forward_cached(sl(a), feats)
        assert torch.equal(got, want) and torch.equal(percept(a, b), want)
    assert all(not f.requires_grad for f in feats) and len(feats) == 5


# ------------------------------------------------------------------------------------------------ the loop
@pytest.mark.parametrize('name', [c['name'] for c in pj.TRAJECTORIES])
def test_learning_rates_are_the_recorded_ones(name, golden):
    """_adjust_learning_rate over iterations + 1 steps gives exactly the rates the reference's optimize set, 0 at both
    ends."""
    from Evaluation.image_projection import project
    c = pj.TRAJECTORY_BY_NAME[name]
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.Adam([p], lr=pj.LR)
    got = []
    for i in range(c['iterations'] + 1):
        project._adjust_learning_rate(i, c['iterations'], pj.LR, opt)
        got.append(opt.param_groups[0]['lr'])
    want = golden('projection')[name + '/lr']
    assert np.array_equal(np.array(got), want) and got[0] == 0.0 and abs(got[-1]) < 1e-18


def _run_trajectory(c, g, percept, device='cpu'):
    from Evaluation.image_projection import project
    avg_w, noises, target = pj.trajectory_start(c, g, device=device)
    start = [avg_w.clone()] + [n.clone() for n in noises]
    crit = project.ImageReconstructionLoss(device=device, loss='mse+lpips', percept=percept)
    opt = torch.optim.Adam([avg_w] + noises, lr=pj.LR)
    kwargs = {'noise_z': None, 'input_is_latent': True, 'latent_styles': [avg_w], 'noise': noises}
    history = []
    last = project.optimize(model=g, input_kwargs=kwargs, targets={'target': target, 'mask': None}, criterion=crit,
                            optimizer=opt, iterations=c['iterations'], print_iterations=0, device=device, history=history)
    disp = [(p.detach() - s).double().cpu() for p, s in zip([avg_w] + noises, start)]
    return history, last, disp, crit


def test_toy_trajectory_reproduces_the_reference(golden, percept):
    """optimize + ImageReconstructionLoss('mse+lpips') + Adam with the toy generator on the CPU: the per-step losses within
    4 x |loss32 - loss64| + 2e-6 |loss64| of the reference's float64 run, and the displacement of W and of each noise map
    within 4 x the reference's own relative L2 figure + 2e-6; the target went through the trunk once."""
    c = pj.TRAJECTORY_BY_NAME['toy']
    g = golden('projection')
    trunk = []
    hook = percept.net.net.register_forward_hook(lambda m, i, o: trunk.append(1))
    try:
        history, last, disp, crit = _run_trajectory(c, pj.ToyProjGenerator(), percept)
    finally:
        hook.remove()
    assert len(trunk) == c['iterations'] + 2                       # the target once, the image in every step
    losses = np.array([float(l) for _, l in history])
    l32, l64 = g['toy/loss'], g['toy/loss64']
    gate = 4 * np.abs(l32 - l64) + FLOOR * np.abs(l64)
    print('toy losses', losses, 'loss64', l64, 'err', np.abs(losses - l64), 'gate', gate)
    assert np.all(np.abs(losses - l64) <= gate) and float(last) == pytest.approx(losses[-1])
    assert [lr for lr, _ in history] == list(g['toy/lr'])
    want = [g['toy/dW64']] + [g[f'toy/dnoise{i}64'] for i in range(2)]
    ref_err = [float(g['toy/dW_err'])] + list(g['toy/dnoise_err'])
    for d, w, e in zip(disp, want, ref_err):
        err = np.linalg.norm(pj.noise_sample(d).numpy() - w) / np.linalg.norm(w)
        print('toy displacement rel L2', err, 'reference', e)
        assert err <= 4 * e + FLOOR


def test_optimize_runs_torch_lbfgs_and_refuses_other_optimisers():
    from Evaluation.image_projection import project
    g = pj.ToyProjGenerator()
    c = pj.TRAJECTORY_BY_NAME['toy']
    avg_w, noises, target = pj.trajectory_start(c, g)
    kwargs = {'noise_z': None, 'input_is_latent': True, 'latent_styles': [avg_w], 'noise': noises}
    crit = project.ImageReconstructionLoss(device='cpu', loss='mse')
    first = float(crit(g(**kwargs), {'target': target, 'mask': None}))
    opt = torch.optim.LBFGS([avg_w] + noises, lr=1, max_iter=4)
    history = []
    project.optimize(g, kwargs, {'target': target, 'mask': None}, crit, opt, 2, print_iterations=0, history=history)
    assert len(history) == 3 and avg_w.requires_grad and all(n.requires_grad for n in noises)
    with torch.no_grad():
        assert float(crit(g(**kwargs), {'target': target, 'mask': None})) < first
    with pytest.raises(ValueError, match='Unsupported optimizer'):
        project.optimize(g, kwargs, {'target': target, 'mask': None}, crit, object(), 2)


# ------------------------------------------------------------------------------------------------ the surface
def test_image_projector_on_the_cpu():
    """Image_Projector with the toy generator, from a tensor, a PIL image and a list of them: two CPU tensors of the
    target's shape, the projected one nearer to the target; the generator's parameters, flags and mode are as before;
    opt='LBFGS' raises NotImplementedError and names FullBatchLBFGS."""
    from PIL import Image
    from Evaluation.image_projection import image_projector as IP, project
    g = pj.ToyProjGenerator()
    g.noise_weight.requires_grad_(True)
    g.train()
    before = {k: v.clone() for k, v in g.state_dict().items()}
    target = 0.5 * pj.trajectory_start(pj.TRAJECTORY_BY_NAME['toy'], g)[2]
    crit = project.ImageReconstructionLoss(device='cpu', loss='mse')
    torch.manual_seed(3)
    inp, out = IP.Image_Projector(g, 'cpu', False, target, 'Adam', num_iters=20, print_iters=0, criterion=crit)
    assert inp.shape == out.shape == target.shape and inp.device.type == out.device.type == 'cpu'
    assert not inp.requires_grad and not out.requires_grad
    assert float(((out - target) ** 2).mean()) < float(((inp - target) ** 2).mean())
    assert all(torch.equal(v, before[k]) for k, v in g.state_dict().items())
    assert g.training and g.noise_weight.requires_grad and not g.to_image.weight.requires_grad
    u8 = ((target[0].permute(1, 2, 0) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).numpy()
    wrapped = torch.nn.Module()
    wrapped.module = g
    wrapped.forward = lambda **kw: g(**kw)
    for images, batch, per_layer in ((Image.fromarray(u8), 1, True), ([Image.fromarray(u8)] * 2, 2, False)):
        inp, out = IP.Image_Projector(wrapped, 'cpu', per_layer, images, 'Adam', num_iters=2, print_iters=0,
                                      criterion=project.ImageReconstructionLoss(device='cpu', loss='mse'))
        assert tuple(inp.shape) == tuple(out.shape) == (batch, 3, 16, 16)
    t = IP.img_transform([u8], 'cpu')
    assert torch.equal(t, (torch.from_numpy(u8).permute(2, 0, 1)[None].float() / 255 - 0.5) / 0.5)
    with pytest.raises(NotImplementedError, match='FullBatchLBFGS'):
        IP.Image_Projector(g, 'cpu', False, target, 'LBFGS', criterion=crit)
    assert tuple(IP.Get_Avg_W_as_Latent(g, 'cpu', True).shape) == (1, 3, pj.TOY_DIM)
    assert tuple(IP.Get_Avg_W_as_Latent(g, 'cpu', False).shape) == (1, pj.TOY_DIM)


def test_helpers_reproduce_the_reference(golden):
    from Evaluation.image_projection import image_projector as IP
    g = golden('projection')
    for i in range(2):
        a, b = pj.image_pair(i)
        assert IP.psnr(pj.to_255(a), pj.to_255(b)) == pytest.approx(float(g[f'helpers/psnr/{i}']), rel=1e-12)
        down = IP.Downsample_Image_256(pj.down_input(i))
        assert tuple(down.shape) == (1, 3, 256, 256)
        assert float(np.abs(down[:, :, ::9, ::9].numpy() - g[f'helpers/down/{i}']).max()) <= 2.0 ** -22
    a, b = pj.image_pair(0)
    assert IP.psnr(pj.to_255(a), pj.to_255(a)) == 100 == float(g['helpers/psnr/equal'])
    scores = IP.Get_PSNR_Model_Image([pj.to_255(b), pj.to_255(a)], [pj.to_255(a)])
    assert scores == [[pytest.approx(float(g['helpers/psnr/0']))], [100.0]]
    seen = []

    def standin(x, y):
        seen.append((tuple(x.shape), tuple(y.shape)))
        return ((x - y) ** 2).mean()
    lp = IP.Get_LPIPS_Model_Image([b, a], [a], standin)
    assert seen == [((1, 3, 256, 256),) * 2] * 2 and lp[1] == [0.0] and lp[0][0] > 0
