"""The fused path of FullBatchLBFGS.step on the GPU (csrc/lbfgs.hip, op/lbfgs.py): the Gram-space direction from recorded
and from synthetic states, the pair / gather / update kernels bit for bit against their torch expressions, the ring,
every fixture trajectory, the launches of a step, and Image_Projector(opt='FullBatchLBFGS') on the narrow Generator.

Gates: the standing one (lbfgs_cases.gate); written vectors bit-equal; scalar sums against float64 torch at 1e-12
of sum |a_i b_i|.
"""
import numpy as np
import pytest
import torch

import launches
import lbfgs_cases as lc
import projection_cases as pj
from gpumem import dev, misaligned

pytestmark = pytest.mark.gpu

SEGMENTS = {144: [int(np.prod(s)) for s in lc.SHAPES],
            4099: [1, 3, 16, 4079]}        # odd sizes, misaligned starts, a tail shorter than a vector, three blocks


def make_params(n, seed=0, none_grad=None):
    """Parameters of SEGMENTS[n] with random values and gradients (gradient `none_grad` left None), each in a view that
    starts one float into its storage."""
    gen = torch.Generator().manual_seed(seed)
    params = []
    for i, size in enumerate(SEGMENTS[n]):
        p = misaligned(torch.randn(size, generator=gen).to(dev())).requires_grad_(True)
        if i != none_grad:
            p.grad = misaligned(torch.randn(size, generator=gen).to(dev()))
        params.append(p)
    return params


def flat_grad(params):
    return torch.cat([torch.zeros_like(p).reshape(-1) if p.grad is None else p.grad.reshape(-1) for p in params])


def set_grads(params, flat):
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].clone().view_as(p)
        off += p.numel()


def synthetic_pairs(n, k, seed):
    """k pairs with s.y > 0 (y = a positive diagonal times s, plus a little noise), as float32 CPU tensors."""
    gen = torch.Generator().manual_seed(seed)
    S = torch.randn(k, n, generator=gen) * 0.1
    Y = S * (0.5 + torch.rand(n, generator=gen)) + 0.01 * torch.randn(k, n, generator=gen)
    return S, Y


def composite_direction(S, Y, g, h_diag, device):
    from Evaluation.image_projection import LBFGS
    opt = LBFGS.LBFGS([torch.zeros(g.numel(), device=device, requires_grad=True)])
    state = opt.state['global_state']
    state['old_dirs'] = [s.to(device).clone() for s in S]
    state['old_stps'] = [y.to(device).clone() for y in Y]
    state['H_diag'] = float(h_diag)
    return opt.two_loop_recursion(-g.to(device).clone())


def fused_direction(n, S, Y, g, h_diag, history_size=10):
    from op import lbfgs
    params = make_params(n)
    set_grads(params, g.to(dev()))
    fs = lbfgs.FusedState(params, history_size)
    fs.load(list(S.to(dev())), list(Y.to(dev())), h_diag)
    accepted, h = fs.direction(0.0, 1e-2, False)
    assert not accepted and h == float(h_diag) and fs.count == len(S)
    assert torch.equal(fs.g, g.to(dev())) and torch.equal(fs.g_prev, fs.g)
    exact = float(fs.g.double().dot(fs.d.double()))
    assert abs(fs.gtd - exact) <= 1e-12 * float((fs.g.double() * fs.d.double()).abs().sum()), (fs.gtd, exact)
    return fs.d.clone()


def check_direction(tag, d_fused, S, Y, g, h_diag, d64, dev_ref):
    d_comp = composite_direction(S, Y, g, h_diag, dev()).cpu().numpy()
    err, bound = lc.gate(d_fused.cpu().numpy(), d64, dev_ref)
    dev_c = np.abs(d_comp.astype(np.float64) - d64).max()
    err_c, bound_c = lc.gate(d_fused.cpu().numpy(), d_comp, max(dev_ref, dev_c))
    print(f'{tag}: fused - fp64 {err:.3e} (gate {bound:.3e}), fused - composite {err_c:.3e} (gate {bound_c:.3e})')
    assert err <= bound and err_c <= bound_c, (tag, err, bound, err_c, bound_c)


def test_direction_from_recorded_states(golden):
    """k = 0, 1, 3, 10 live pairs of the reference's float32 run at n = 144, against its float64 direction."""
    g = golden('lbfgs')
    ks = []
    for j in lc.CASES['rosenbrock']['states']:
        st = {k: g[f'rosenbrock/state{j}/{k}'] for k in ('S', 'Y', 'g', 'd', 'd64', 'H_diag')}
        S, Y, grad = torch.from_numpy(st['S']), torch.from_numpy(st['Y']), torch.from_numpy(st['g'])
        ks.append(len(S))
        d = fused_direction(144, S, Y, grad, float(st['H_diag']))
        check_direction(f'state {j} k {len(S)}', d, S, Y, grad, float(st['H_diag']), st['d64'],
                        np.abs(st['d'].astype(np.float64) - st['d64']).max())
    assert {0, 1, 3, 10} <= set(ks)


@pytest.mark.parametrize('k', [0, 1, 3, 10])
def test_direction_from_synthetic_states(k):
    """n = 4099 in segments of 1, 3, 16 and 4079 elements; the deviation of the gate is the CPU composite's (the
    reference's operations in float32) from the float64 recursion."""
    n = 4099
    S, Y = synthetic_pairs(n, k, seed=k)
    grad = torch.randn(n, generator=torch.Generator().manual_seed(100 + k))
    h_diag = 0.7
    d64 = lc.two_loop_f64(S.numpy(), Y.numpy(), grad.numpy(), h_diag)
    dev_ref = np.abs(composite_direction(S, Y, grad, h_diag, 'cpu').numpy().astype(np.float64) - d64).max()
    d = fused_direction(n, S, Y, grad, h_diag)
    check_direction(f'n {n} k {k}', d, S, Y, grad, h_diag, d64, dev_ref)


def _close(got, a, b, what):
    """A kernel's float64 sum against torch's float64 product of the float32 vectors a, b: 1e-12 of sum |a_i b_i|."""
    a, b = a.double(), b.double()
    want, scale = float(a.dot(b)), float((a * b).abs().sum())
    assert abs(got - want) <= 1e-12 * scale, (what, got, want, scale)


@pytest.mark.parametrize('n', [144, 4099])
def test_pair_gather_update_kernels(n):
    """The written vectors bit for bit against t * d, g - g_prev and p + a * d (torch's add with alpha, a fused
    multiply-add on this device as the kernel's), one gradient None; the sums against float64 torch."""
    from op import _native, lbfgs
    m, k, t, a = 10, 3, 0.37, -0.8125
    params = make_params(n, seed=n, none_grad=1)
    fs = lbfgs.FusedState(params, m)
    S, Y = synthetic_pairs(n, k, seed=7)
    gen = torch.Generator().manual_seed(11)
    g_prev, d = torch.randn(n, generator=gen).to(dev()), torch.randn(n, generator=gen).to(dev())
    fs.load(list(S.to(dev())), list(Y.to(dev())), 1.0, g_prev=g_prev, d=d)
    grad = flat_grad(params)
    table, nseg = _native.lbfgs_segments(params)
    assert nseg == 4 and table[4] == 0
    _native.lbfgs_pair(fs, table, nseg, t, True)
    cand = (fs.head + 1) % (m + 1)
    s_want, y_want = d.mul(t), grad.sub(g_prev)
    assert torch.equal(fs.g, grad) and torch.equal(fs.S[cand], s_want) and torch.equal(fs.Y[cand], y_want)
    assert torch.equal(fs.S[:k], S.to(dev())) and torch.equal(fs.Y[:k], Y.to(dev())) and torch.equal(fs.g_prev, g_prev)
    _native.lbfgs_coeffs(fs, t, 1e-2, True)
    rec = fs.record.tolist()
    _close(rec[lbfgs.REC_YS], y_want, s_want, 'ys')
    _close(rec[lbfgs.REC_YY], y_want, y_want, 'yy')
    _close(rec[lbfgs.REC_GG], grad, grad, 'gg')
    _close(rec[lbfgs.REC_SBS] / -float(np.float32(t)), s_want, g_prev, 'sBs')
    accepted = rec[lbfgs.REC_YS] > float(np.float32(1e-2)) * rec[lbfgs.REC_SBS]
    assert (rec[lbfgs.REC_ACCEPTED] == 1.0) == accepted
    G = fs.G.cpu()
    gi = 2 * (m + 1)
    rows = {gi: grad}
    if accepted:
        rows.update({cand: s_want, m + 1 + cand: y_want})
    cols = dict(rows)
    cols.update({i: fs.S[i] for i in range(k)})
    cols.update({m + 1 + i: fs.Y[i] for i in range(k)})
    for r, vr in rows.items():
        for c, vc in cols.items():
            _close(float(G[r, c]), vr, vc, ('G', r, c))
            assert float(G[r, c]) == float(G[c, r])
    # gather: the same table, into g_new, with g_new . d
    fs.d.copy_(d)
    g_new, gtd_new = fs.gather()
    assert torch.equal(g_new, grad)
    _close(gtd_new, grad, d, 'g_new.d')
    # update: through the table, the storage around the parameters untouched
    before = [p.detach().clone() for p in params]
    fs.update(a)
    off = 0
    for p, b in zip(params, before):
        want = b.add(d[off:off + p.numel()].view_as(b), alpha=a)
        ulp = (p.detach().view(torch.int32) - want.view(torch.int32)).abs().max().item()
        print(f'n {n} update segment of {p.numel()}: max distance from torch {ulp} ulp')
        assert torch.equal(p.detach(), want)
        off += p.numel()


def test_ring_rejection_and_wrap_around():
    """history_size 3 with a full ring: a rejected pair leaves every live slot as it was; accepted pairs wrap around and
    old_dirs / old_stps come out in the composite's order, bit for bit."""
    from Evaluation.image_projection import LBFGS
    from op import lbfgs
    n, m = 4099, 3
    params = make_params(n, seed=5)
    fs = lbfgs.FusedState(params, m)
    S, Y = synthetic_pairs(n, m, seed=9)
    d0 = torch.randn(n, generator=torch.Generator().manual_seed(13)).to(dev())
    fs.load(list(S.to(dev())), list(Y.to(dev())), 1.0, g_prev=-d0, d=d0)
    comp = LBFGS.LBFGS([torch.zeros(n, device=dev(), requires_grad=True)], history_size=m)
    cs = comp.state['global_state']
    cs['old_dirs'], cs['old_stps'] = [s.clone() for s in S.to(dev())], [y.clone() for y in Y.to(dev())]
    S0, Y0, state0 = fs.S.clone(), fs.Y.clone(), fs.state.clone()
    live = fs.slots()
    # y = -0.1 d against s = d: y.s < 0 <= eps * sBs = eps * |d|^2, rejected
    set_grads(params, fs.g_prev - 0.1 * fs.d)
    accepted, _ = fs.direction(1.0, 1e-2, True)
    assert not accepted and fs.slots() == live and torch.equal(fs.state[:2], state0[:2])
    assert torch.equal(fs.S[live], S0[live]) and torch.equal(fs.Y[live], Y0[live])
    assert fs.last[lbfgs.REC_YS] < 0 < fs.last[lbfgs.REC_SBS]
    for step in range(5):       # accepted pairs: y = 0.5 s with s = t d, sBs = -t s.g_prev
        t = 0.5 + 0.25 * step
        d_now, g_prev_now = fs.d.clone(), fs.g_prev.clone()
        grad = g_prev_now + 0.5 * t * d_now
        set_grads(params, grad)
        cs.update({'fail': False, 'd': d_now, 't': t, 'prev_flat_grad': g_prev_now, 'Bs': g_prev_now.mul(-t)})
        comp.curvature_update(grad.clone())
        accepted, h_diag = fs.direction(t, 1e-2, True)
        assert accepted and fs.count == m and fs.state[:2].tolist() == [fs.head, fs.count]
        assert fs.state[2:2 + m].tolist() == fs.slots()
        old_dirs, old_stps = fs.history()
        assert len(old_dirs) == len(cs['old_dirs']) == m
        for ours, theirs in zip(old_dirs + old_stps, cs['old_dirs'] + cs['old_stps']):
            assert torch.equal(ours, theirs), step
        assert h_diag == pytest.approx(float(cs['H_diag']), rel=1e-5)


_runs = {}


def fused_run(name):
    from Evaluation.image_projection import LBFGS
    if name not in _runs:
        rec, _, opt = lc.run_case(lc.CASES[name], LBFGS.FullBatchLBFGS, torch.float32, device=dev())
        assert opt._fused is not None
        _runs[name] = rec
    return _runs[name]


@pytest.mark.parametrize('name', sorted(lc.CASES))
def test_fixture_trajectories_on_the_fused_path(golden, name):
    """Every fixture case on the kernels: the decisions of the reference at every step, loss and iterate inside the gate;
    a second run gives the same bits."""
    from Evaluation.image_projection import LBFGS
    rec = fused_run(name)
    lc.check_trajectory(golden('lbfgs'), name, rec, 'fused')
    again, _, _ = lc.run_case(lc.CASES[name], LBFGS.FullBatchLBFGS, torch.float32, device=dev())
    for key in ('x', 'loss', 't'):
        assert np.array_equal(rec[key], again[key]), (name, key)


def _counted_step(monkeypatch, fuse):
    """The launches of the third step of the convex case under the Wolfe search, and the step's return."""
    from Evaluation.image_projection import LBFGS
    monkeypatch.setattr(LBFGS, 'FUSE', fuse)
    case = dict(lc.CASES['none'], line_search='Wolfe', lr=1, steps=2)
    _, _, opt = lc.run_case(case, LBFGS.FullBatchLBFGS, torch.float32, device=dev())
    params = opt._params

    def closure():
        opt.zero_grad()
        return lc.quartic_bowl(params)

    loss = closure()
    loss.backward()
    with launches.observed() as seen:
        out = opt.step({'closure': closure, 'current_loss': loss})
    return seen, out, opt


def test_launches_of_a_step(monkeypatch):
    seen, out, opt = _counted_step(monkeypatch, True)
    assert out[3] == 0 and not out[7] and opt._fused is not None      # accepted at the first trial
    assert seen.names == ['lbfgs_pair', 'lbfgs_coeffs', 'lbfgs_direction', 'lbfgs_update', 'lbfgs_gather']
    seen, out, opt = _counted_step(monkeypatch, False)
    assert out[3] == 0 and opt._fused is None
    assert not [n for n in seen.names if n.startswith('lbfgs')]


def test_image_projector_full_batch_lbfgs_on_the_generator(monkeypatch):
    """Generator(64), W+, B = 2, 4 iterations: the loss falls, the Generator is unwritten, and the projected image equals
    the composite's within the gate, whose deviation is the composite's own answer to a change of the last bit of the
    target (both are float32 runs; there is no float64 Generator to take the deviation from)."""
    from Evaluation.image_projection import LBFGS, image_projector as IP, project
    from test_projection_gpu import _generator
    gen = _generator(64)
    before = {k: v.clone() for k, v in gen.state_dict().items()}
    target = pj.trajectory_start(pj.TRAJECTORY_BY_NAME['g64_wplus'], gen, device=dev())[2]
    assert target.shape[0] == 2

    def run(fuse, tgt):
        monkeypatch.setattr(LBFGS, 'FUSE', fuse)
        torch.manual_seed(7)
        with launches.observed() as seen:
            inp, out = IP.Image_Projector(gen, dev(), True, tgt, 'FullBatchLBFGS', num_iters=4, print_iters=0,
                                          criterion=project.ImageReconstructionLoss(device=dev(), loss='mse'))
        return inp, out, seen.count('lbfgs_direction')

    inp, out, fused_steps = run(True, target)
    _, out_c, composite_steps = run(False, target)
    _, out_p, _ = run(False, target * (1 + 2.0 ** -23))
    assert fused_steps == 5 and composite_steps == 0
    t = target.cpu()
    first, last = float(((inp - t) ** 2).mean()), float(((out - t) ** 2).mean())
    err, bound = lc.gate(out.numpy(), out_c.numpy(), np.abs(out_p.numpy().astype(np.float64) - out_c.numpy()).max())
    print(f'mse {first:.4e} -> {last:.4e}; fused - composite {err:.3e}, gate {bound:.3e}')
    assert last < first
    assert err <= bound
    assert all(torch.equal(v, before[k]) for k, v in gen.state_dict().items())
