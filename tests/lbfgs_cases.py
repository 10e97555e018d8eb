"""Cases of the L-BFGS tests, shared by tools/make_golden_lbfgs.py (which runs them on the reference's optimiser and
writes tests/golden/lbfgs.npz) and by tests/test_lbfgs.py / test_lbfgs_gpu.py (which run them on this project's).

The objectives are closed-form torch functions of a list of parameter tensors: no networks.  run_case drives any class with
FullBatchLBFGS's interface the way project.optimize does and records, per step, the loss, the step length, the line
search's counters and the flat iterate, and, at the steps of case['states'], the state the direction was computed from.
"""
import numpy as np
import torch

SHAPES = ((2, 3, 8), (1, 1, 4, 4), (1, 1, 4, 4), (1, 1, 8, 8))          # 144 elements in four tensors


def _flat(params):
    return torch.cat([p.reshape(-1) for p in params])


def rosenbrock(params):
    x = _flat(params)
    return (100 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2).sum()


def double_well(params):
    """Non-convex: negative curvature around 0, wells near +-1, a weak coupling of neighbours."""
    x = _flat(params)
    return (0.25 * (x ** 2 - 1) ** 2).sum() + 0.1 * (x[1:] * x[:-1]).sum() + 0.05 * x.sum()


def quartic_bowl(params):
    """Convex and well conditioned: a step of fixed length converges."""
    x = _flat(params)
    a = torch.linspace(1, 3, x.numel(), dtype=x.dtype, device=x.device)
    return (0.5 * a * x ** 2).sum() + 0.25 * (x ** 4).sum() + 0.1 * (x[1:] * x[:-1]).sum()


OBJECTIVES = {'rosenbrock': rosenbrock, 'double_well': double_well, 'quartic_bowl': quartic_bowl}

# name -> objective, seed and scale of the start, optimiser arguments, extra options, steps, steps whose state is kept
CASES = {
    'rosenbrock': dict(objective='rosenbrock', seed=1, scale=0.05, shift=0.8, steps=26, states=(0, 1, 3, 12, 25)),
    'nonconvex': dict(objective='double_well', seed=8, scale=0.3, steps=12, options={'eps': 0.5}, wants='curv_skips'),
    'ls_fail': dict(objective='double_well', seed=4, scale=0.6, steps=10, options={'eps': 0.3, 'max_ls': 1},
                    wants='fail'),
    'history3': dict(objective='rosenbrock', seed=3, scale=0.1, shift=0.5, steps=12, history_size=3),
    'history1': dict(objective='rosenbrock', seed=3, scale=0.1, shift=0.5, steps=8, history_size=1),
    'armijo': dict(objective='rosenbrock', seed=3, scale=0.1, shift=0.5, steps=10, line_search='Armijo'),
    'none': dict(objective='quartic_bowl', seed=9, scale=0.5, steps=8, line_search='None', lr=0.5),
}
DECISIONS = ('ls_step', 'closure_eval', 'grad_eval', 'desc_dir', 'fail', 'history')


def start(case, dtype, device='cpu'):
    gen = torch.Generator().manual_seed(case['seed'])
    return [(torch.randn(s, generator=gen, dtype=torch.float64) * case['scale'] + case.get('shift', 0.0))
            .to(dtype=dtype, device=device) for s in SHAPES]


def run_case(case, optimizer_class, dtype, device='cpu', params=None):
    """Runs the case; returns (records, states, optimizer): records[key] is a list over the steps, states[j] the dict
    {'S', 'Y', 'g', 'H_diag', 'd'} of step j (numpy, in the run's dtype)."""
    objective = OBJECTIVES[case['objective']]
    line_search = case.get('line_search', 'Wolfe')
    params = start(case, dtype, device) if params is None else params
    for p in params:
        p.requires_grad_(True)
    opt = optimizer_class(params, lr=case.get('lr', 1), history_size=case.get('history_size', 10),
                          line_search=line_search, dtype=dtype)

    def closure():
        opt.zero_grad()
        return objective(params)

    loss = closure()
    loss.backward()
    rec = {k: [] for k in ('loss', 't', 'x') + DECISIONS}
    states = {}
    for j in range(case['steps']):
        options = {'closure': closure, 'current_loss': loss}
        options.update(case.get('options', {}))
        out = opt.step(options)
        ls_step = closure_eval = grad_eval = 0
        desc_dir, fail = True, False
        if line_search == 'Wolfe':
            loss, _, t, ls_step, closure_eval, grad_eval, desc_dir, fail = out
        elif line_search == 'Armijo':
            loss, t, ls_step, closure_eval, desc_dir, fail = out
            loss.backward()
        else:
            t = out
            loss = closure()
            loss.backward()
        state = opt.state['global_state']
        rec['loss'].append(float(loss.detach()))
        rec['t'].append(float(t))
        rec['x'].append(_flat(params).detach().cpu().numpy().copy())
        for k, v in zip(DECISIONS, (ls_step, closure_eval, grad_eval, desc_dir, fail, len(state['old_dirs']))):
            rec[k].append(int(v))
        if j in case.get('states', ()):
            n = rec['x'][-1].size
            stack = lambda vs: (torch.stack([v.detach().cpu() for v in vs]).numpy() if len(vs)      # noqa: E731
                                else np.zeros((0, n), rec['x'][-1].dtype))
            states[j] = {'S': stack(state['old_dirs']), 'Y': stack(state['old_stps']),
                         'g': state['prev_flat_grad'].detach().cpu().numpy().copy(),
                         'H_diag': float(state['H_diag']), 'd': state['d'].detach().cpu().numpy().copy()}
    rec = {k: np.asarray(v) for k, v in rec.items()}
    rec['curv_skips'] = int(opt.state['global_state']['curv_skips'])
    rec['fail_skips'] = int(opt.state['global_state']['fail_skips'])
    return rec, states, opt


def two_loop_f64(S, Y, g, h_diag):
    """The two-loop recursion in float64 on the given pairs (oldest first): the direction -H g, as a numpy vector."""
    S, Y, q = np.asarray(S, np.float64), np.asarray(Y, np.float64), -np.asarray(g, np.float64)
    k = len(S)
    rho = [1.0 / Y[i].dot(S[i]) for i in range(k)]
    alpha = [0.0] * k
    for i in range(k - 1, -1, -1):
        alpha[i] = S[i].dot(q) * rho[i]
        q = q - alpha[i] * Y[i]
    r = q * float(h_diag)
    for i in range(k):
        beta = Y[i].dot(r) * rho[i]
        r = r + (alpha[i] - beta) * S[i]
    return r


# polyinterp inputs of the kinds the line searches produce: two points with three or four known values
POLYINTERP = (
    ([[0.0, 1.5, -2.0], [1.0, 1.2, np.nan]], None, None),
    ([[0.5, 1.5, -2.0], [2.0, 3.0, np.nan]], None, None),
    ([[0.0, 1.0, -1.0], [1.0, 0.9, 0.5]], None, None),
    ([[0.0, 1.0, -1.0], [2.0, 0.2, 0.3]], 0.1, 1.2),
    ([[0.3, 2.0, -4.0], [0.9, 1.0, 3.0]], None, None),
)


def gate(ours, ref64, dev, scale=None):
    """The standing gate: |ours - ref64| <= 4 * dev + 2e-6 * max |value|; dev: the reference's own
    fp32-vs-fp64 deviation.  Returns (error, bound)."""
    ours, ref64 = np.asarray(ours, np.float64), np.asarray(ref64, np.float64)
    scale = float(np.max(np.abs(ref64))) if scale is None else scale
    return float(np.max(np.abs(ours - ref64))) if ours.size else 0.0, 4 * float(dev) + 2e-6 * scale


def check_trajectory(g, name, rec, dtype_name='f32'):
    """rec (of lc.run_case) against the fixture `name`: decisions equal, loss and iterate inside the gate at every step."""
    for k in DECISIONS:
        assert np.array_equal(rec[k], g[f'{name}/{k}']), (name, k, rec[k].tolist(), g[f'{name}/{k}'].tolist())
    assert [rec['curv_skips'], rec['fail_skips']] == g[f'{name}/skips'].tolist(), name
    worst = 0.0
    for key in ('loss', 'x', 't'):
        r32, r64 = g[f'{name}/{key}/f32'].astype(np.float64), g[f'{name}/{key}/f64']
        ours = rec[key].astype(np.float64)
        assert ours.shape == r64.shape
        dev = 0.0
        for j in range(len(r64)):
            dev = max(dev, float(np.abs(r32[j] - r64[j]).max()))
            err, bound = gate(ours[j], r64[j], dev)
            assert err <= bound, (name, key, j, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    print(f'{name} [{dtype_name}]: worst error / bound {worst:.3f}')
    return worst
