"""The loss log of train() without a host synchronisation per iteration (csrc/train_loop.hip fmgan_loss_row_f32,
DESIGN 3.4m).

The reference's Print_Train_Status (train_3_encoder.py:636-655) calls reduce_loss_dict and then .item() nine times
after every iteration: nine collectives and nine host synchronisations, so the host never runs ahead of the device.  A
LossLedger keeps a ring of rows on the device; an iteration costs one launch that gathers the nine scalars into the
next row and two event records, and the host reads the ring back once per `rows` iterations: one device-to-host copy,
one event synchronise and — with more than one rank — ONE reduce of the whole block to rank 0.

On a CPU device the row is torch.stack and the time the host clock: the host logic runs without a GPU.
"""
import time

import torch

from Miscellaneous import distributed as D_

from . import _native

NAMES = ('d', 'r1', 'g_reg', 'g', 'lpips', 'l1', 'face_id', 'hmap', 'face_reg')
COLUMNS = _native.LOSS_ROW_COLUMNS


class LossLedger:
    def __init__(self, device, rows, extra_names=()):
        self.names = tuple(NAMES) + tuple(extra_names)
        if len(self.names) > COLUMNS or len(set(self.names)) != len(self.names):
            raise ValueError(f'LossLedger: {len(self.names)} columns ({COLUMNS} at most, each name once)')
        if int(rows) < 1:
            raise ValueError(f'LossLedger: rows = {rows}')
        self.device = torch.device(device)
        self.rows = int(rows)
        self.gpu = self.device.type == 'cuda'
        self.ring = torch.zeros((self.rows, COLUMNS), dtype=torch.float32, device=self.device)
        if self.gpu:
            if self.device.index is None:
                self.device = torch.device('cuda', torch.cuda.current_device())
            self.host = torch.zeros((self.rows, COLUMNS), dtype=torch.float32).pin_memory()
            self.events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                           for _ in range(self.rows)]
            self.copied = torch.cuda.Event()
        else:
            self.host = self.ring
            self.events = [[0.0, 0.0] for _ in range(self.rows)]
        self.meta = [None] * self.rows
        self.used = 0
        self.begun = False
        self.flushes = 0            # flushes that returned at least one row

    def full(self):
        return self.used >= self.rows

    def begin(self):
        """The start of an iteration's time, on the current stream."""
        if self.full():
            raise RuntimeError('LossLedger: the ring is full; flush() first')
        if self.gpu:
            self.events[self.used][0].record(torch.cuda.current_stream(self.device))
        else:
            self.events[self.used][0] = time.perf_counter()
        self.begun = True

    def _value(self, v):
        if v is None:
            return None
        if torch.is_tensor(v):
            v = v.detach()
            if v.numel() > 1:
                v = v.mean()
            if v.dtype == torch.float32 and v.device == self.device and v.numel() == 1:
                return v
        return torch.as_tensor(v, dtype=torch.float32, device=self.device).reshape(())

    def write(self, iter_idx, loss_dict, ds_flag, extreme_ds_flag):
        """The end of the iteration's time and its row: one launch of the detached values' addresses."""
        if self.full():
            raise RuntimeError('LossLedger: the ring is full; flush() first')
        if not self.begun:
            self.begin()
        k = self.used
        values = [self._value(loss_dict.get(name)) for name in self.names]
        if self.gpu:
            self.events[k][1].record(torch.cuda.current_stream(self.device))
            _native.loss_row(values, self.ring[k])
        else:
            self.events[k][1] = time.perf_counter()
            zero = torch.zeros((), dtype=torch.float32)
            row = torch.stack([zero if v is None else v.reshape(()) for v in values])
            self.ring[k, :len(values)] = row
            self.ring[k, len(values):] = 0
        self.meta[k] = (int(iter_idx), bool(ds_flag), bool(extreme_ds_flag))
        self.used = k + 1
        self.begun = False

    def flush(self):
        """The pending rows, oldest first, as (iter_idx, seconds, ds_flag, extreme_ds_flag, {name: float}); empties the
        ring.  With more than one rank the values are the mean over ranks and only rank 0 returns them."""
        n = self.used
        if n == 0:
            return []
        world = D_.get_world_size()
        block = self.ring[:n]
        if world > 1:
            torch.distributed.reduce(block, dst=0, op=torch.distributed.ReduceOp.SUM)
        self.used, self.begun = 0, False
        if D_.get_rank() != 0:
            return []
        if self.gpu:
            self.host[:n].copy_(block, non_blocking=True)
            self.copied.record(torch.cuda.current_stream(self.device))
            self.copied.synchronize()
            seconds = [start.elapsed_time(end) * 1e-3 for start, end in self.events[:n]]
        else:
            seconds = [end - start for start, end in self.events[:n]]
        table = self.host[:n]
        if world > 1:
            table = table / world
        table = table.tolist()
        out = []
        for k in range(n):
            iter_idx, ds_flag, extreme_ds_flag = self.meta[k]
            out.append((iter_idx, seconds[k], ds_flag, extreme_ds_flag, dict(zip(self.names, table[k]))))
        self.flushes += 1
        return out
