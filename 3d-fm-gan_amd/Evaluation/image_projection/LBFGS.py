"""L-BFGS with Armijo / Armijo-Wolfe line searches for the image projection (the reference's third-party
Evaluation/image_projection/LBFGS.py: `is_legal`, `polyinterp`, `LBFGS`, `FullBatchLBFGS`), written anew.

    is_legal, polyinterp   :19-154    the quadratic and cubic closed forms the line searches reach, bisection otherwise
    LBFGS                  :159-990   two_loop_recursion, curvature_update, step(p_k, g_Ok, g_Sk, options)
    FullBatchLBFGS         :995-1122  step(options): gradient, curvature update, direction and line search in one call

Two implementations behind one interface:
  * the composite: plain torch on flat tensors, the reference's operations in the reference's order (any device and
    dtype).  LBFGS.step, two_loop_recursion and curvature_update always use it;
  * the fused path (op/lbfgs.py, csrc/lbfgs.hip): FullBatchLBFGS.step keeps g, the previous gradient, the
    direction and the (s, y) ring in flat float32 buffers and computes the direction in Gram space, five kinds of launch per
    step.  It is taken when fused_declined() answers None; anything else takes the composite, silently.

Kept from the reference, on purpose: the argument checks, the options, the return tuples (Wolfe eight values, Armijo
six, 'None' the step length), the keys of state['global_state'] and their swapped names: `old_dirs` holds the steps s and
`old_stps` the gradient differences y, oldest first.
What is different, on purpose:
  * polyinterp has no plotting and no linear solve: the line searches hand it two points with (f, g) and (f) or (f, g)
    known, every other input is answered by bisection;
  * the NaN placeholders of the line searches are host floats (the reference builds device tensors for them);
  * on the fused path state['H_diag'] and the step lengths are host floats, state['Bs'] does not exist (sBs is
    -t * s.g_prev), state['d'] / state['prev_flat_grad'] and the entries of old_dirs / old_stps are views of the
    optimiser's own buffers, and the g_new of the Wolfe tuple is such a buffer too: valid until the next step.
"""
import os
from copy import deepcopy
from functools import reduce

import numpy as np
import torch
from torch.optim import Optimizer

# FullBatchLBFGS.step on the HIP kernels where they serve; False keeps the torch composite.
FUSE = os.environ.get('FMGAN_NO_LBFGS_FUSE', '0') != '1'
MAX_FUSED_HISTORY = 32      # csrc/lbfgs.hip: the Gram matrix of 2 * 32 + 1 vectors fits one block's shared memory
MAX_FUSED_PARAMS = 64       # the segment table travels to the kernels by value


def _value(v):
    return v.item() if torch.is_tensor(v) else float(v)


def is_legal(v):
    """True when v (a tensor or a number) holds neither NaN nor Inf."""
    v = torch.as_tensor(v)
    return not bool(torch.isnan(v).any()) and not bool(torch.isinf(v).any())


def polyinterp(points, x_min_bound=None, x_max_bound=None):
    """Minimiser of the polynomial through `points` (rows [x, f, g], NaN for an unknown f or g) inside
    [x_min_bound, x_max_bound] (default: the range of x).  Two points with three known values: the quadratic closed form;
    with four: the cubic one; anything else, or a cubic without a real critical point: the midpoint of the bounds."""
    points = np.asarray(points, dtype=np.float64)
    no_points = points.shape[0]
    order = int(np.sum(1 - np.isnan(points[:, 1:3]).astype('int'))) - 1
    if x_min_bound is None:
        x_min_bound = np.min(points[:, 0])
    if x_max_bound is None:
        x_max_bound = np.max(points[:, 0])
    if no_points == 2 and order == 2:
        (x1, f1, g1), (x2, f2, _) = points
        if x1 == 0:
            x_sol = -g1 * x2 ** 2 / (2 * (f2 - f1 - g1 * x2))
        else:
            a = -(f1 - f2 - g1 * (x1 - x2)) / (x1 - x2) ** 2
            x_sol = x1 - g1 / (2 * a)
        return np.minimum(np.maximum(x_min_bound, x_sol), x_max_bound)
    if no_points == 2 and order == 3:
        (x1, f1, g1), (x2, f2, g2) = points
        d1 = g1 + g2 - 3 * ((f1 - f2) / (x1 - x2))
        with np.errstate(invalid='ignore'):
            d2 = np.sqrt(d1 ** 2 - g1 * g2)
        if np.isreal(d2):       # a negative discriminant gives NaN here, which is "real": so does the reference
            x_sol = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2))
            return np.minimum(np.maximum(x_min_bound, x_sol), x_max_bound)
    return (x_min_bound + x_max_bound) / 2


def fused_declined(params, dtype=torch.float, history_size=10, damping=False):
    """Why FullBatchLBFGS.step would take the composite for these parameters (host logic, nothing runs): a string, or
    None when the fused path serves them."""
    params = list(params)
    if not FUSE:
        return 'LBFGS.FUSE is off'
    if damping:
        return 'Powell damping'
    if dtype != torch.float:
        return f'dtype {dtype}'
    if not 1 <= history_size <= MAX_FUSED_HISTORY:
        return f'history_size {history_size} outside 1..{MAX_FUSED_HISTORY}'
    if not 1 <= len(params) <= MAX_FUSED_PARAMS:
        return f'{len(params)} parameters, 1..{MAX_FUSED_PARAMS} are served'
    for p in params:
        for what, v in (('parameter', p), ('gradient', p.grad)):
            if v is None:
                continue
            if not v.is_cuda or v.device != params[0].device:
                return f'a {what} on {v.device}'
            if v.dtype != torch.float32 or v.is_sparse or not v.is_contiguous():
                return f'a {what} that is not a contiguous float32 tensor'
    if sum(p.numel() for p in params) == 0:
        return 'no elements'
    return None


class LBFGS(Optimizer):
    """L-BFGS on one parameter group: the caller supplies the direction p_k and the gradients, step() runs the line
    search ('Wolfe', 'Armijo' or 'None') and records what curvature_update and two_loop_recursion need next."""

    def __init__(self, params, lr=1, history_size=10, line_search='Wolfe', dtype=torch.float, debug=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0 <= history_size:
            raise ValueError("Invalid history size: {}".format(history_size))
        if line_search not in ['Armijo', 'Wolfe', 'None']:
            raise ValueError("Invalid line search: {}".format(line_search))
        defaults = dict(lr=lr, history_size=history_size, line_search=line_search, dtype=dtype, debug=debug)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("L-BFGS doesn't support per-parameter options (parameter groups)")
        self._params = self.param_groups[0]['params']
        self._numel_cache = None
        self._fused = None          # op.lbfgs.FusedState while FullBatchLBFGS.step runs on the kernels
        state = self.state['global_state']
        state.setdefault('n_iter', 0)
        state.setdefault('curv_skips', 0)
        state.setdefault('fail_skips', 0)
        state.setdefault('H_diag', 1)
        state.setdefault('fail', True)
        state['old_dirs'] = []
        state['old_stps'] = []

    # ------------------------------------------------------------------------------------------ flat views
    def _numel(self):
        if self._numel_cache is None:
            self._numel_cache = reduce(lambda total, p: total + p.numel(), self._params, 0)
        return self._numel_cache

    def _gather_flat_grad(self):
        views = []
        for p in self._params:
            if p.grad is None:
                views.append(p.data.new(p.data.numel()).zero_())
            elif p.grad.data.is_sparse:
                views.append(p.grad.data.to_dense().view(-1))
            else:
                views.append(p.grad.data.view(-1))
        return torch.cat(views, 0)

    def _add_update(self, step_size, update):
        if self._fused is not None:
            return self._fused.update(step_size)
        offset = 0
        for p in self._params:
            numel = p.numel()
            p.data.add_(update[offset:offset + numel].view_as(p.data), alpha=step_size)
            offset += numel
        assert offset == self._numel()

    def _gradient_along(self, d):
        """(flat gradient at the trial point, its product with d) for the curvature condition."""
        if self._fused is not None:
            return self._fused.gather()
        g_new = self._gather_flat_grad()
        return g_new, g_new.dot(d)

    def _copy_params(self):
        return [deepcopy(p.data) for p in self._params]

    def _load_params(self, current_params):
        for p, saved in zip(self._params, current_params):
            p.data[:] = saved

    def line_search(self, line_search):
        """Switches the line search: 'None', 'Armijo' or 'Wolfe'."""
        self.param_groups[0]['line_search'] = line_search

    # ------------------------------------------------------------------------------------------ composite algebra
    def two_loop_recursion(self, vec):
        """H vec by the two-loop recursion over the stored pairs; `vec` is overwritten."""
        history_size = self.param_groups[0]['history_size']
        state = self.state['global_state']
        old_dirs = state.get('old_dirs')    # the steps s
        old_stps = state.get('old_stps')    # the gradient differences y
        H_diag = state.get('H_diag')
        num_old = len(old_dirs)
        if 'rho' not in state:
            state['rho'] = [None] * history_size
            state['alpha'] = [None] * history_size
        rho, alpha = state['rho'], state['alpha']
        for i in range(num_old):
            rho[i] = 1. / old_stps[i].dot(old_dirs[i])
        q = vec
        for i in range(num_old - 1, -1, -1):
            alpha[i] = old_dirs[i].dot(q) * rho[i]
            q.add_(old_stps[i], alpha=-alpha[i])
        r = torch.mul(q, H_diag)
        for i in range(num_old):
            beta = old_stps[i].dot(r) * rho[i]
            r.add_(old_dirs[i], alpha=alpha[i] - beta)
        return r

    def curvature_update(self, flat_grad, eps=1e-2, damping=False):
        """Stores the pair (s, y) = (t d, flat_grad - previous gradient) unless the last line search failed or
        y.s <= eps * s.Bs (with damping: the Powell-damped y instead of a rejection)."""
        assert len(self.param_groups) == 1
        if eps <= 0:
            raise ValueError('Invalid eps; must be positive.')
        group = self.param_groups[0]
        history_size, debug = group['history_size'], group['debug']
        state = self.state['global_state']
        if state.get('fail'):
            state['fail_skips'] += 1
            if debug:
                print('Line search failed; curvature pair update skipped')
            return
        old_dirs, old_stps = state.get('old_dirs'), state.get('old_stps')
        Bs = state.get('Bs')
        y = flat_grad.sub(state.get('prev_flat_grad'))
        s = state.get('d').mul(state.get('t'))
        sBs = s.dot(Bs)
        ys = y.dot(s)
        if ys > eps * sBs or damping:
            if damping and ys < eps * sBs:
                if debug:
                    print('Applying Powell damping...')
                theta = ((1 - eps) * sBs) / (sBs - ys)
                y = theta * y + (1 - theta) * Bs
            if len(old_dirs) == history_size:
                old_dirs.pop(0)
                old_stps.pop(0)
            old_dirs.append(s)
            old_stps.append(y)
            state['old_dirs'] = old_dirs
            state['old_stps'] = old_stps
            state['H_diag'] = ys / y.dot(y)
        else:
            state['curv_skips'] += 1
            if debug:
                print('Curvature pair skipped due to failed criterion')

    # ------------------------------------------------------------------------------------------ line searches
    @staticmethod
    def _options(options, wolfe):
        if not options:
            raise ValueError('Options are not specified; need closure evaluating function.')
        if 'closure' not in options:
            raise ValueError('closure option not specified.')
        o = {'eta': 2, 'c1': 1e-4, 'c2': 0.9, 'max_ls': 10, 'interpolate': True, 'inplace': True, 'ls_debug': False}
        o.update({k: options[k] for k in o if k in options})
        if 'eta' in options and wolfe and o['eta'] <= 1:
            raise ValueError('Invalid eta; must be greater than 1.')
        if 'eta' in options and not wolfe and o['eta'] <= 0:
            raise ValueError('Invalid eta; must be positive.')
        if o['c1'] >= 1 or o['c1'] <= 0:
            raise ValueError('Invalid c1; must be strictly between 0 and 1.')
        if wolfe and (o['c2'] >= 1 or o['c2'] <= 0):
            raise ValueError('Invalid c2; must be strictly between 0 and 1.')
        if wolfe and 'c2' in options and o['c2'] <= o['c1']:
            raise ValueError('Invalid c2; must be strictly larger than c1.')
        if o['max_ls'] <= 0:
            raise ValueError('Invalid max_ls; must be positive.')
        return o

    def _step(self, p_k, g_Ok, g_Sk=None, options={}, device=None):
        assert len(self.param_groups) == 1
        group = self.param_groups[0]
        lr, line_search, debug = group['lr'], group['line_search'], group['debug']
        state = self.state['global_state']
        fused = self._fused is not None
        state['n_iter'] += 1
        d = p_k
        t = lr
        closure_eval = 0
        if fused:       # the direction launch has copied g into the previous-gradient buffer; there is no Bs
            prev_flat_grad = self._fused.g_prev
        else:
            prev_flat_grad = state.get('prev_flat_grad')
            if prev_flat_grad is None:
                prev_flat_grad = g_Ok.clone()
            else:
                prev_flat_grad.copy_(g_Ok)
            if g_Sk is None:
                g_Sk = g_Ok.clone()

        def finish(t, fail):
            if not fused:
                Bs = state.get('Bs')
                if Bs is None:
                    Bs = (g_Sk.mul(-t)).clone()
                else:
                    Bs.copy_(g_Sk.mul(-t))
                state['Bs'] = Bs
            state['d'] = d
            state['prev_flat_grad'] = prev_flat_grad
            state['t'] = t
            state['fail'] = fail

        if line_search == 'None':
            self._add_update(t, d)
            finish(t, False)
            return t

        wolfe = line_search == 'Wolfe'
        o = self._options(options, wolfe)
        closure = options['closure']
        eta, c1, c2, max_ls = o['eta'], o['c1'], o['c2'], o['max_ls']
        interpolate, inplace, ls_debug = o['interpolate'], o['inplace'], o['ls_debug'] and debug

        def default_gtd():
            return self._fused.gtd if fused else g_Ok.dot(d)

        if wolfe:
            if 'current_loss' not in options:
                F_k = closure()
                closure_eval += 1
            else:
                F_k = options['current_loss']
            gtd = options['gtd'] if 'gtd' in options else default_gtd()
        else:
            gtd = options['gtd'] if 'gtd' in options else default_gtd()
            if 'current_loss' not in options:
                F_k = closure()
                closure_eval += 1
            else:
                F_k = options['current_loss']

        ls_step = 0
        t_prev = 0
        fail = False
        if ls_debug:
            print('Begin %s line search  F(x): %.8e  g*d: %.8e' % (line_search, _value(F_k), _value(gtd)))
        if gtd >= 0:
            desc_dir = False
            if debug:
                print('Not a descent direction!')
        else:
            desc_dir = True
        if not inplace:
            current_params = self._copy_params()

        def move(t_to, t_from):
            if inplace:
                self._add_update(t_to - t_from, d)
            else:
                self._load_params(current_params)
                self._add_update(t_to, d)

        self._add_update(t, d)
        F_new = closure()
        closure_eval += 1

        if not wolfe:
            F_prev = float('nan')
            while F_new > F_k + c1 * t * gtd or not is_legal(F_new):
                if ls_step >= max_ls:
                    if inplace:
                        self._add_update(-t, d)
                    else:
                        self._load_params(current_params)
                    t = 0
                    F_new = closure()
                    closure_eval += 1
                    fail = True
                    break
                t_new = t
                if ls_step == 0 or not interpolate or not is_legal(F_new):
                    t = t / eta
                elif ls_step == 1 or not is_legal(F_prev):
                    t = polyinterp(np.array([[0, _value(F_k), _value(gtd)], [t_new, _value(F_new), np.nan]]))
                else:
                    t = polyinterp(np.array([[0, _value(F_k), _value(gtd)], [t_new, _value(F_new), np.nan],
                                             [t_prev, _value(F_prev), np.nan]]))
                if interpolate:
                    if t < 1e-3 * t_new:
                        t = 1e-3 * t_new
                    elif t > 0.6 * t_new:
                        t = 0.6 * t_new
                    F_prev = F_new
                    t_prev = t_new
                move(t, t_new)
                F_new = closure()
                closure_eval += 1
                ls_step += 1
                if ls_debug:
                    print('LS Step: %d  t: %.8e  F(x+td): %.8e' % (ls_step, t, _value(F_new)))
            finish(t, fail)
            return F_new, t, ls_step, closure_eval, desc_dir, fail

        grad_eval = 0
        alpha = 0
        beta = float('Inf')
        F_a, g_a = F_k, gtd
        F_b, g_b = float('nan'), float('nan')
        while True:
            if ls_step >= max_ls:
                if inplace:
                    self._add_update(-t, d)
                else:
                    self._load_params(current_params)
                t = 0
                F_new = closure()
                F_new.backward()
                g_new, _ = self._gradient_along(d)
                closure_eval += 1
                grad_eval += 1
                fail = True
                break
            if ls_debug:
                print('LS Step: %d  t: %.8e  alpha: %.8e  beta: %.8e  F(x+td): %.8e' % (ls_step, t, alpha, beta,
                                                                                        _value(F_new)))
            if F_new > F_k + c1 * t * gtd:
                beta = t
                t_prev = t
                if interpolate:
                    F_b, g_b = F_new, float('nan')
            else:
                F_new.backward()
                g_new, gtd_new = self._gradient_along(d)
                grad_eval += 1
                if gtd_new < c2 * gtd:
                    alpha = t
                    t_prev = t
                    if interpolate:
                        F_a, g_a = F_new, gtd_new
                else:
                    break
            if not interpolate or not is_legal(F_b):
                if beta == float('Inf'):
                    t = eta * t
                else:
                    t = (alpha + beta) / 2.0
            else:
                t = polyinterp(np.array([[alpha, _value(F_a), _value(g_a)], [beta, _value(F_b), _value(g_b)]]))
                if beta == float('Inf'):
                    if t > 2 * eta * t_prev:
                        t = 2 * eta * t_prev
                    elif t < eta * t_prev:
                        t = eta * t_prev
                else:
                    if t < alpha + 0.2 * (beta - alpha):
                        t = alpha + 0.2 * (beta - alpha)
                    elif t > (beta - alpha) / 2.0:
                        t = (beta - alpha) / 2.0
                if t <= 0:
                    t = (beta - alpha) / 2.0
            move(t, t_prev)
            F_new = closure()
            closure_eval += 1
            ls_step += 1
        finish(t, fail)
        return F_new, g_new, t, ls_step, closure_eval, grad_eval, desc_dir, fail

    def step(self, p_k, g_Ok, g_Sk=None, options={}):
        """One line search along p_k from the current iterate.  g_Ok: the flat gradient the next curvature pair is
        differenced against; g_Sk (default g_Ok): the one the rejection criterion uses.  Returns what the line search
        returns (see the module docstring).  Always the composite."""
        self._leave_fused()
        return self._step(p_k, g_Ok, g_Sk, options)

    # ------------------------------------------------------------------------------------------ fused state
    def _leave_fused(self):
        """Hands the fused path's state to the composite (an option of a later step asked for it)."""
        fs, self._fused = self._fused, None
        if fs is None:
            return
        state = self.state['global_state']
        state['old_dirs'] = [s.clone() for s in state['old_dirs']]
        state['old_stps'] = [y.clone() for y in state['old_stps']]
        state['d'] = fs.d.clone()
        state['prev_flat_grad'] = fs.g_prev.clone()
        state['Bs'] = fs.g_prev.mul(-float(state.get('t') or 0))
        state['H_diag'] = torch.tensor(float(state['H_diag']), dtype=torch.float32, device=fs.d.device)


class FullBatchLBFGS(LBFGS):
    """Deterministic L-BFGS: step(options) reads the parameters' gradients, updates the curvature pairs, computes the
    direction and runs the line search.  options: 'eps' (1e-2) and 'damping' (False) of the curvature update, and the
    line search's 'closure', 'current_loss', 'gtd', 'eta', 'c1', 'c2', 'max_ls', 'interpolate', 'inplace', 'ls_debug'."""

    def __init__(self, params, lr=1, history_size=10, line_search='Wolfe', dtype=torch.float, debug=False):
        super().__init__(params, lr, history_size, line_search, dtype, debug)

    def _serves_fused(self, damping):
        group = self.param_groups[0]
        state = self.state['global_state']
        if self._fused is None and state['n_iter'] > 0:     # the composite has begun: its state stays where it is
            return False
        return fused_declined(self._params, group['dtype'], group['history_size'], damping) is None

    def step(self, options={}, device=None):
        damping = options['damping'] if 'damping' in options else False
        eps = options['eps'] if 'eps' in options else 1e-2
        state = self.state['global_state']
        if not self._serves_fused(damping):
            self._leave_fused()
            grad = self._gather_flat_grad()
            if state['n_iter'] > 0:
                self.curvature_update(grad, eps, damping)
            p = self.two_loop_recursion(-grad)
            return self._step(p, grad, options=options, device=device)

        if self._fused is None:
            from op import lbfgs as fused_ops
            self._fused = fused_ops.FusedState(self._params, self.param_groups[0]['history_size'])
        fs = self._fused
        has_pair = False
        if state['n_iter'] > 0:
            if eps <= 0:
                raise ValueError('Invalid eps; must be positive.')
            has_pair = not state['fail']
            if not has_pair:
                state['fail_skips'] += 1
        accepted, h_diag = fs.direction(float(state.get('t') or 0) if has_pair else 0.0, float(eps), has_pair)
        if has_pair:
            if accepted:
                state['H_diag'] = h_diag
            else:
                state['curv_skips'] += 1
        state['old_dirs'], state['old_stps'] = fs.history()
        return self._step(fs.d, fs.g, options=options, device=device)
