"""The EMA of a parameter set in one launch (csrc/train_loop.hip fmgan_ema_f32).

`accumulate` (Util/training_util.py) is a mul_ and an add_ per parameter: 164 / 220 / 276 aten launches per iteration
for Generator(64 / 256 / 1024).  An EmaPlan pairs the parameters of the two modules by name once, keeps a device table of
{dst, src, numel, block_begin} and launches one kernel per update.  Buffers (the fixed noise maps) are not averaged,
exactly as in `accumulate`.

The table holds raw pointers, so every update first compares the recorded data_ptr() and numel() of each pair with the
live ones and rebuilds the table when any changed: load_state_dict copies in place and keeps them, `.to()` / `.half()`
give the parameters new storage.

There is no fallback here: inputs the kernel does not take are refused (RuntimeError); a caller that wants the composite
asks EmaPlan.declined first (Util.training_util.accumulate_fused does) — the contract of op/lbfgs.py.
"""
import numpy as np
import torch

from . import _native

_ENTRY = np.dtype([('dst', '<u8'), ('src', '<u8'), ('numel', '<i8'), ('block_begin', '<i8')])


def _pairs(model1, model2):
    return dict(model1.named_parameters()), dict(model2.named_parameters())


def table_for(pairs):
    """(table, n_entries, total_blocks, numel) of fmgan_ema_f32 for (dst, src) tensor pairs that have passed the checks
    of EmaPlan.declined: the table a uint8 tensor on the pairs' device (None when there is no pair)."""
    rows, blocks, numel = [], 0, 0
    for p, q in pairs:
        rows.append((p.data_ptr(), q.data_ptr(), p.numel(), blocks))
        blocks += _native.ema_blocks(p.numel())
        numel += p.numel()
    if not rows:
        return None, 0, 0, 0
    table = np.array(rows, dtype=_ENTRY)
    return torch.from_numpy(table.view(np.uint8).copy()).to(pairs[0][0].device), len(rows), blocks, numel


class EmaPlan:
    """model1 <- decay * model1 + (1 - decay) * model2 over named_parameters(), one launch per update()."""

    def __init__(self, model1, model2):
        reason = EmaPlan.declined(model1, model2)
        if reason is not None:
            raise RuntimeError(f'op.ema: {reason}')
        self.model1, self.model2 = model1, model2
        self.rebuilds = 0
        self._key = None
        self._table = None
        self._n = self._blocks = self._numel = 0
        self._build()

    @staticmethod
    def declined(model1, model2):
        """Why the kernel does not take this pair of modules — a string — or None."""
        par1, par2 = _pairs(model1, model2)
        if list(par1) != list(par2):
            odd = sorted(set(par1) ^ set(par2))
            return f'different parameter names ({odd[:3] if odd else "another order"})'
        device = None
        for k, p in par1.items():
            q = par2[k]
            if tuple(p.shape) != tuple(q.shape):
                return f'different shapes of {k}: {tuple(p.shape)} and {tuple(q.shape)}'
            for t in (p, q):
                if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                    return (f'{k} is not a contiguous float32 CUDA tensor ({t.dtype} on {t.device}, strides '
                            f'{tuple(t.stride())})')
                if device is None:
                    device = t.device
                elif t.device != device:
                    return f'{k} is on {t.device}, other parameters on {device}'
        # no dst may share a byte with a src (the kernel reads and writes them in no order), nor with another dst
        spans = []
        for k, p in par1.items():
            if p.numel():
                spans.append((p.data_ptr(), p.data_ptr() + 4 * p.numel(), 0, k))
                q = par2[k]
                spans.append((q.data_ptr(), q.data_ptr() + 4 * q.numel(), 1, k))
        spans.sort()
        end = [(0, None), (0, None)]            # furthest end seen of a dst span / of a src span, and whose it is
        for lo, hi, is_src, k in spans:
            for other in ((0,) if is_src else (0, 1)):
                if lo < end[other][0]:
                    return f'overlapping storage between {end[other][1]} and {k}'
            if hi > end[is_src][0]:
                end[is_src] = (hi, k)
        return None

    def _live_key(self):
        par1, par2 = _pairs(self.model1, self.model2)
        return tuple((p.data_ptr(), p.numel()) for p in par1.values()) + \
            tuple((q.data_ptr(), q.numel()) for q in par2.values())

    def _build(self, key=None):
        par1, par2 = _pairs(self.model1, self.model2)
        self._table, self._n, self._blocks, self._numel = table_for([(p, par2[k]) for k, p in par1.items()])
        self._key = self._live_key() if key is None else key
        self.rebuilds += 1

    def update(self, decay):
        """One launch on the current stream of the parameters' device, under no_grad."""
        key = self._live_key()
        if key != self._key:
            reason = EmaPlan.declined(self.model1, self.model2)
            if reason is not None:
                raise RuntimeError(f'op.ema: {reason}')
            self._build(key)
        if self._table is None or self._blocks == 0:
            return
        with torch.no_grad():
            _native.ema(self._table, self._n, self._blocks, decay, self._numel)
