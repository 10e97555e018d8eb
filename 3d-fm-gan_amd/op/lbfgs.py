"""Device state and launches of the fused L-BFGS step (csrc/lbfgs.hip): what
Evaluation/image_projection/LBFGS.py's FullBatchLBFGS.step runs on when LBFGS.fused_declined() answers None.

The state is flat float32: g, g_prev, d, g_new of n elements and a ring of history_size + 1 slots each for the steps S and
the gradient differences Y (the spare slot receives the candidate pair, so a rejected pair never overwrites a live one).
The parameters and their gradients keep their own storage and are reached through a segment table.  The Gram matrix G of
the ring's vectors and g is kept in float64 on the device between steps; every step adds only the rows of the new s, y
and g.  The host reads one 64-byte record per step and per trial gradient.

There is no fallback here: tensors the kernels do not take are refused (RuntimeError); the caller asks
LBFGS.fused_declined first and evaluates the composite itself.
"""
import torch

from . import _native

REC_ACCEPTED, REC_HDIAG, REC_YS, REC_SBS, REC_GTD, REC_GTD_NEW, REC_GG, REC_YY = range(8)
MAX_HISTORY = 32
MAX_PARAMS = 64
STREAM_BLOCKS = 2048        # csrc/lbfgs.hip LB_STREAM_BLOCKS


class FusedState:
    def __init__(self, params, history_size):
        self.params = list(params)
        if not 1 <= len(self.params) <= MAX_PARAMS or not 1 <= history_size <= MAX_HISTORY:
            raise RuntimeError(f'op.lbfgs: {len(self.params)} parameters (1..{MAX_PARAMS}) and history_size '
                               f'{history_size} (1..{MAX_HISTORY})')
        _native.require_f32_gpu('op.lbfgs', tuple((p, 'a parameter') for p in self.params))
        dev = self.params[0].device
        self.n = n = sum(p.numel() for p in self.params)
        self.m = m = int(history_size)
        if n == 0:
            raise RuntimeError('op.lbfgs: no elements')
        f32 = dict(dtype=torch.float32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.g, self.g_prev, self.d, self.g_new = (torch.zeros(n, **f32) for _ in range(4))
        self.S = torch.zeros((m + 1, n), **f32)
        self.Y = torch.zeros((m + 1, n), **f32)
        dim = 2 * (m + 1) + 1
        self.G = torch.zeros((dim, dim), **f64)
        self.coef = torch.zeros(dim, **f64)
        self.record = torch.zeros(8, **f64)
        self.record[REC_HDIAG] = 1.0
        self.state = torch.zeros(m + 2, dtype=torch.int32, device=dev)
        blocks = int(_native.lib().fmgan_lbfgs_pair_blocks(n))
        if blocks <= 0:
            raise RuntimeError(f'op.lbfgs: {n} elements are more than a grid holds')
        self.partial = torch.zeros(max(blocks * (6 * m + 7), STREAM_BLOCKS), **f64)
        self.head, self.count = 0, 0        # the host's mirror of state[0:2]
        self.gtd = 0.0
        self.last = None                    # the record read after the last direction launch

    def _table(self):
        for p in self.params:
            if p.grad is not None:
                _native.require_f32_gpu('op.lbfgs', ((p.grad, 'a gradient'),))
                if p.grad.device != self.g.device or p.grad.numel() != p.numel():
                    raise RuntimeError('op.lbfgs: a gradient on another device or of another size than its parameter')
        return _native.lbfgs_segments(self.params)

    def direction(self, t, eps, has_pair):
        """One step's algebra: pair, coeffs, direction; returns (accepted, H_diag) and leaves g.d in self.gtd."""
        table, nseg = self._table()
        _native.lbfgs_pair(self, table, nseg, t, has_pair)
        _native.lbfgs_coeffs(self, t, eps, has_pair)
        _native.lbfgs_direction(self)
        self.last = rec = self.record.tolist()
        accepted = rec[REC_ACCEPTED] != 0.0
        if accepted:
            self.head = (self.head + 1) % (self.m + 1)
            self.count = min(self.count + 1, self.m)
        self.gtd = rec[REC_GTD]
        return accepted, rec[REC_HDIAG]

    def slots(self):
        """The live slots, oldest first."""
        return [(self.head - self.count + 1 + i) % (self.m + 1) for i in range(self.count)]

    def history(self):
        live = self.slots()
        return [self.S[j] for j in live], [self.Y[j] for j in live]

    def update(self, a):
        table, nseg = _native.lbfgs_segments(self.params)
        _native.lbfgs_update(self, table, nseg, a)

    def gather(self):
        table, nseg = self._table()
        _native.lbfgs_gather(self, table, nseg)
        return self.g_new, self.record[REC_GTD_NEW].item()

    def load(self, s_list, y_list, h_diag, g_prev=None, d=None):
        """Puts recorded pairs (oldest first) into the ring and rebuilds G from them in float64 (torch, not a hot path):
        restoring a state, and the tests' way in."""
        k = len(s_list)
        if k != len(y_list) or k > self.m:
            raise ValueError(f'op.lbfgs: {k} steps and {len(y_list)} differences for a history of {self.m}')
        self.S.zero_()
        self.Y.zero_()
        self.G.zero_()
        for i in range(k):
            self.S[i].copy_(s_list[i].reshape(-1))
            self.Y[i].copy_(y_list[i].reshape(-1))
        if k:
            basis = torch.cat([self.S[:k], self.Y[:k]]).double()
            gram = basis @ basis.t()
            idx = torch.tensor(list(range(k)) + [self.m + 1 + i for i in range(k)], device=self.G.device)
            self.G[idx[:, None], idx[None, :]] = gram
        self.head, self.count = max(k - 1, 0), k
        state = [self.head, self.count] + list(range(k)) + [0] * (self.m - k)
        self.state.copy_(torch.tensor(state, dtype=torch.int32))
        self.record[REC_HDIAG] = float(h_diag)
        if g_prev is not None:
            self.g_prev.copy_(g_prev.reshape(-1))
        if d is not None:
            self.d.copy_(d.reshape(-1))
