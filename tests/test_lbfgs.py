"""Evaluation/image_projection/LBFGS.py on the CPU: the composite against fixtures recorded from the reference's optimiser
(tools/make_golden_lbfgs.py, tests/golden/lbfgs.npz), polyinterp, the argument checks, the FullBatchLBFGS branch of
project.optimize, Image_Projector(opt='FullBatchLBFGS') and the predicate that chooses between composite and kernels.

The gate is the standing one: at step j the loss and the iterate lie within 4 x the reference's own
float32-vs-float64 deviation (the largest seen up to step j) plus 2e-6 x max |value| of the reference's float64 run.  The
line search's decisions must be equal at every step; no step is excused.
"""
import numpy as np
import pytest
import torch

import lbfgs_cases as lc
import projection_cases as pj


@pytest.mark.parametrize('name', sorted(lc.CASES))
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_composite_follows_the_reference(golden, name, dtype):
    from Evaluation.image_projection import LBFGS
    rec, _, opt = lc.run_case(lc.CASES[name], LBFGS.FullBatchLBFGS, dtype)
    assert opt._fused is None
    lc.check_trajectory(golden('lbfgs'), name, rec, str(dtype))
    state = opt.state['global_state']
    for key in ('n_iter', 'curv_skips', 'fail_skips', 'fail', 't', 'H_diag', 'd', 'prev_flat_grad', 'old_dirs',
                'old_stps'):
        assert key in state, key
    assert state['n_iter'] == lc.CASES[name]['steps']


def test_direction_from_recorded_states(golden):
    """two_loop_recursion on the recorded (S, Y, g, H_diag) of the float32 run against the float64 direction."""
    from Evaluation.image_projection import LBFGS
    g = golden('lbfgs')
    for j in lc.CASES['rosenbrock']['states']:
        st = {k: g[f'rosenbrock/state{j}/{k}'] for k in ('S', 'Y', 'g', 'd', 'd64', 'H_diag')}
        opt = LBFGS.LBFGS([torch.zeros(st['g'].size, requires_grad=True)])
        state = opt.state['global_state']
        state['old_dirs'] = [torch.from_numpy(v) for v in st['S']]
        state['old_stps'] = [torch.from_numpy(v) for v in st['Y']]
        state['H_diag'] = float(st['H_diag'])
        d = opt.two_loop_recursion(-torch.from_numpy(st['g'])).numpy()
        err, bound = lc.gate(d, st['d64'], np.abs(st['d'].astype(np.float64) - st['d64']).max())
        assert err <= bound, (j, err, bound)
        assert np.abs(lc.two_loop_f64(st['S'], st['Y'], st['g'], st['H_diag']) - st['d64']).max() <= 1e-12 * (
            1 + np.abs(st['d64']).max())


def test_polyinterp(golden):
    from Evaluation.image_projection import LBFGS
    g = golden('lbfgs')
    for i, (points, lo, hi) in enumerate(lc.POLYINTERP):
        got = float(LBFGS.polyinterp(np.array(points), lo, hi))
        assert got == pytest.approx(float(g[f'polyinterp/{i}']), rel=1e-14, abs=0), (i, got)
    # anything but two points with three or four known values: the midpoint of the bounds
    three = np.array([[0.0, 1.0, -1.0], [1.0, 1.5, np.nan], [2.0, 4.0, np.nan]])
    assert LBFGS.polyinterp(three) == 1.0 and LBFGS.polyinterp(three, 0.5, 1.0) == 0.75
    assert LBFGS.polyinterp(np.array([[0.0, 1.0, np.nan], [4.0, 2.0, np.nan]])) == 2.0
    assert LBFGS.is_legal(torch.tensor(1.0)) and not LBFGS.is_legal(torch.tensor(float('nan')))
    assert not LBFGS.is_legal(torch.tensor(float('inf'))) and LBFGS.is_legal(0.5)


def test_argument_errors():
    from Evaluation.image_projection import LBFGS
    p = [torch.zeros(4, requires_grad=True)]
    for kw in ({'lr': -1}, {'history_size': -1}, {'line_search': 'Exact'}):
        with pytest.raises(ValueError, match='Invalid'):
            LBFGS.FullBatchLBFGS(p, **kw)
    with pytest.raises(ValueError, match='parameter groups'):
        LBFGS.LBFGS([{'params': p}, {'params': [torch.zeros(2, requires_grad=True)]}])

    def closure():
        return (p[0] ** 2).sum() + 1

    loss = closure()
    loss.backward()
    for ls in ('Wolfe', 'Armijo'):
        opt = LBFGS.FullBatchLBFGS(p, line_search=ls)
        with pytest.raises(ValueError, match='Options are not specified'):
            opt.step({})
        with pytest.raises(ValueError, match='closure option not specified'):
            opt.step({'current_loss': loss})
        bad = [{'c1': 0}, {'c1': 1}, {'max_ls': 0}, {'eta': 0 if ls == 'Armijo' else 1}]
        if ls == 'Wolfe':
            bad += [{'c2': 1}, {'c2': 0}, {'c2': 1e-5}]
        for extra in bad:
            with pytest.raises(ValueError, match='Invalid'):
                LBFGS.FullBatchLBFGS(p, line_search=ls).step(dict({'closure': closure, 'current_loss': loss}, **extra))
    opt = LBFGS.FullBatchLBFGS(p)
    opt.step({'closure': closure, 'current_loss': loss})
    with pytest.raises(ValueError, match='Invalid eps'):
        opt.step({'closure': closure, 'current_loss': loss, 'eps': 0})
    opt.line_search('None')
    assert opt.param_groups[0]['line_search'] == 'None' and opt.step() == 1


def test_options_damping_and_not_inplace():
    """Powell damping keeps every pair; inplace=False restores the parameters from copies and ends at the same iterate as
    the in-place search up to rounding."""
    from Evaluation.image_projection import LBFGS
    case = dict(lc.CASES['nonconvex'], options={'eps': 0.5, 'damping': True})
    rec, _, opt = lc.run_case(case, LBFGS.FullBatchLBFGS, torch.float64)
    assert rec['curv_skips'] == 0 and rec['history'][-1] == min(10, case['steps'] - 1)
    a, _, _ = lc.run_case(lc.CASES['rosenbrock'], LBFGS.FullBatchLBFGS, torch.float64)
    b, _, _ = lc.run_case(dict(lc.CASES['rosenbrock'], options={'inplace': False}), LBFGS.FullBatchLBFGS, torch.float64)
    assert np.array_equal(a['ls_step'], b['ls_step']) and np.abs(a['x'] - b['x']).max() < 1e-9


def _toy_problem():
    from Evaluation.image_projection import project
    g = pj.ToyProjGenerator()
    avg_w, noises, target = pj.trajectory_start(pj.TRAJECTORY_BY_NAME['toy'], g)
    kwargs = {'noise_z': None, 'input_is_latent': True, 'latent_styles': [avg_w], 'noise': noises}
    crit = project.ImageReconstructionLoss(device='cpu', loss='mse')
    return g, avg_w, noises, {'target': target, 'mask': None}, kwargs, crit


def test_optimize_runs_full_batch_lbfgs():
    from Evaluation.image_projection import LBFGS, project
    g, avg_w, noises, targets, kwargs, crit = _toy_problem()
    first = float(crit(g(**kwargs), targets))
    opt = LBFGS.FullBatchLBFGS([avg_w] + noises, lr=1)
    history = []
    last = project.optimize(g, kwargs, targets, crit, opt, 5, print_iterations=0, history=history)
    assert len(history) == 6 and opt.state['global_state']['n_iter'] == 6
    losses = [float(v) for _, v in history]
    assert all(b <= a for a, b in zip([first] + losses, losses)) and losses[-1] < 0.5 * first
    assert float(last) == losses[-1] and all(t >= 0 for t, _ in history)
    with torch.no_grad():
        assert float(crit(g(**kwargs), targets)) == pytest.approx(losses[-1], rel=1e-6)


def test_image_projector_full_batch_lbfgs_on_the_cpu():
    from Evaluation.image_projection import image_projector as IP, project
    g = pj.ToyProjGenerator()
    before = {k: v.clone() for k, v in g.state_dict().items()}
    target = 0.5 * pj.trajectory_start(pj.TRAJECTORY_BY_NAME['toy'], g)[2]
    crit = project.ImageReconstructionLoss(device='cpu', loss='mse')
    torch.manual_seed(3)
    inp, out = IP.Image_Projector(g, 'cpu', False, target, 'FullBatchLBFGS', num_iters=6, print_iters=0, criterion=crit)
    assert inp.shape == out.shape == target.shape and not out.requires_grad
    assert float(((out - target) ** 2).mean()) < 0.5 * float(((inp - target) ** 2).mean())
    assert all(torch.equal(v, before[k]) for k, v in g.state_dict().items())
    with pytest.raises(NotImplementedError, match="opt='FullBatchLBFGS'"):
        IP.Image_Projector(g, 'cpu', False, target, 'LBFGS', criterion=crit)


def test_gating_predicate_is_host_logic(monkeypatch):
    """fused_declined never touches a device: meta tensors stand for the GPU's.  Each departure selects the composite."""
    from Evaluation.image_projection import LBFGS

    def params(count=2, dtype=torch.float32, device='meta'):
        return [torch.empty((3, 5), dtype=dtype, device=device, requires_grad=True) for _ in range(count)]

    class OnGpu(torch.Tensor):       # a meta tensor that answers as a GPU tensor does
        is_cuda = True

    def on_gpu(ps):
        return [p.detach().as_subclass(OnGpu) for p in ps]

    assert LBFGS.fused_declined(on_gpu(params())) is None
    assert 'damping' in LBFGS.fused_declined(on_gpu(params()), damping=True)
    assert 'dtype' in LBFGS.fused_declined(on_gpu(params()), dtype=torch.double)
    assert 'float32' in LBFGS.fused_declined(on_gpu(params(dtype=torch.float64)))
    assert 'history_size' in LBFGS.fused_declined(on_gpu(params()), history_size=33)
    assert LBFGS.fused_declined(on_gpu(params()), history_size=32) is None
    assert 'parameters' in LBFGS.fused_declined(on_gpu(params(65)))
    assert LBFGS.fused_declined(on_gpu(params(64))) is None
    assert 'cpu' in LBFGS.fused_declined(params(device='cpu'))
    strided = on_gpu(params())
    strided[1] = torch.empty((5, 3), device='meta').t().as_subclass(OnGpu)
    assert 'contiguous' in LBFGS.fused_declined(strided)
    monkeypatch.setattr(LBFGS, 'FUSE', False)
    assert 'FUSE' in LBFGS.fused_declined(on_gpu(params()))
    # and the optimiser acts on it: CPU parameters run the composite, no fused state is ever built
    rec, _, opt = lc.run_case(dict(lc.CASES['history1'], steps=2), LBFGS.FullBatchLBFGS, torch.float32)
    assert opt._fused is None


def test_entry_points_check_their_arguments_without_a_gpu():
    """The argument checks of csrc/lbfgs.hip's entry points run before any HIP call: statuses, no launch."""
    import ctypes
    from nets import lib
    L = lib()
    assert L.fmgan_lbfgs_pair_blocks(0) == 0 and L.fmgan_lbfgs_pair_blocks(1) == 1
    assert L.fmgan_lbfgs_pair_blocks(2048) == 1 and L.fmgan_lbfgs_pair_blocks(2049) == 2
    assert L.fmgan_lbfgs_pair_blocks(2805392) == 1370 and L.fmgan_lbfgs_pair_blocks(1 << 50) == 0
    table = (ctypes.c_longlong * 6)(64, 0, 5, 128, 0, 3)
    seg = ctypes.addressof(table)
    ok = [64] * 7       # non-null stand-ins; no launch is reached below
    assert L.fmgan_lbfgs_pair_f32(None, 2, *ok, 8, 10, 1.0, 0, None) == -1             # no table
    assert L.fmgan_lbfgs_pair_f32(seg, 0, *ok, 8, 10, 1.0, 0, None) == -1              # nseg outside 1..64
    assert L.fmgan_lbfgs_pair_f32(seg, 65, *ok, 8, 10, 1.0, 0, None) == -1
    assert L.fmgan_lbfgs_pair_f32(seg, 2, *ok, 9, 10, 1.0, 0, None) == -1              # numels do not add up to n
    assert L.fmgan_lbfgs_pair_f32(seg, 2, None, *ok[1:], 8, 10, 1.0, 0, None) == -1    # null g
    assert L.fmgan_lbfgs_pair_f32(seg, 2, *ok, 8, 33, 1.0, 0, None) == -2              # history beyond 32
    assert L.fmgan_lbfgs_pair_f32(seg, 2, *ok, 8, 0, 1.0, 0, None) == -2
    assert L.fmgan_lbfgs_coeffs_f64(None, 64, 64, 64, 64, 8, 10, 1.0, 0.01, 0, None) == -1
    assert L.fmgan_lbfgs_coeffs_f64(64, 64, 64, 64, 64, 8, 33, 1.0, 0.01, 0, None) == -2
    assert L.fmgan_lbfgs_direction_f32(*([64] * 8), None, 8, 10, None) == -1
    assert L.fmgan_lbfgs_direction_f32(*([64] * 9), 0, 10, None) == -1
    assert L.fmgan_lbfgs_update_f32(seg, 2, None, 1.0, 8, None) == -1
    assert L.fmgan_lbfgs_update_f32(seg, 2, 64, 1.0, 7, None) == -1
    assert L.fmgan_lbfgs_gather_f32(seg, 2, 64, 64, 64, None, 8, None) == -1
    bad = (ctypes.c_longlong * 3)(0, 0, 8)                                              # elements without a parameter
    assert L.fmgan_lbfgs_gather_f32(ctypes.addressof(bad), 1, 64, 64, 64, 64, 8, None) == -1
