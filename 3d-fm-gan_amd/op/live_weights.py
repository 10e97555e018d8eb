"""Derived weights that are never stale: one `fmgan_weight_refresh_f32` launch per inference forward.

The reference recomputes `weight * scale` / `bias * lr_mul` in every EqualLinear call and the modulated weights in
every ModulatedConv2d call (stylegan2.py:165-175, 257-262).  Round 1 of this build cached those derived tensors under
no_grad, keyed on the parameter's autograd version — but an in-place update through `.data` (the reference's EMA
`accumulate`, train_3_encoder.py:195-200, and `.data.copy_()`-style checkpoint loaders) changes neither the version
nor the storage pointer, so g_ema kept synthesising from the weights of its first call.  There is no reliable
invalidation signal, so nothing is cached across forwards any more: a network owns persistent derived BUFFERS and a
device-side table (source parameter -> buffer), and its inference forward starts by re-deriving all of them from the
live storage in one launch (~240 MB of traffic for Generator(1024): tens of microseconds on MI355X, against the ~90
elementwise launches per forward the reference spends).  Outside such a forward (a bare StyledConv call, training with
autograd) every module derives what it needs on the spot.
"""
import weakref

import numpy as np
import torch

from . import _native

_ENTRY = np.dtype([('src', '<u8'), ('dst', '<u8'), ('dst2', '<u8'), ('dst3', '<u8'), ('n', '<i8'), ('kind', '<i4'),
                   ('cout', '<i4'), ('cin', '<i4'), ('ktaps', '<i4'), ('scale', '<f4'), ('block_begin', '<u4')])
WINOGRAD_MIN_CHANNELS = 256     # stylegan2.winograd_pays: cin, cout >= 256


def _check_layout():
    if _native.lib().fmgan_refresh_entry_bytes() != _ENTRY.itemsize:
        raise RuntimeError('fmgan_refresh_entry layout mismatch between libfmgan_hip.so and op/live_weights.py')


class LiveWeights:
    """Derived-weight buffers of every EqualLinear / 3x3 ModulatedConv2d below `root`."""

    def __init__(self, root):
        self.root = root
        self.active = False
        self._key = None
        self._table = None
        self._blocks = 0
        self._n = 0
        self._buffers = []

    def __deepcopy__(self, memo):
        """A copy of the network (g_ema = deepcopy(G)) starts WITHOUT table and buffers: the copied table would still
        hold the raw pointers of the original's parameters and buffers, and the pointer key alone does not protect a
        copy whose parameters later land on the original's old addresses."""
        import copy
        new = LiveWeights.__new__(LiveWeights)
        memo[id(self)] = new
        new.__init__(copy.deepcopy(self.root, memo))
        return new

    def _sources(self):
        from stylegan2 import EqualLinear, ModulatedConv2d
        lin, conv = [], []
        for m in self.root.modules():
            if isinstance(m, EqualLinear):
                lin.append(m)
            elif isinstance(m, ModulatedConv2d) and m.kernel_size == 3:
                conv.append(m)
        return lin, conv

    def _build(self, lin, conv, key):
        from stylegan2 import WINOGRAD
        _check_layout()
        rows, bufs = [], []
        blocks = 0

        def add(kind, src, dst, dst2, cout, cin, ktaps, scale, n, dst3=None):
            nonlocal blocks
            nb = _native.lib().fmgan_weight_refresh_blocks(kind, cout, cin, ktaps, n)
            if nb <= 0:
                raise RuntimeError('live_weights: unsupported entry')
            rows.append((src.data_ptr(), dst.data_ptr(), 0 if dst2 is None else dst2.data_ptr(),
                         0 if dst3 is None else dst3.data_ptr(), n, kind, cout, cin, ktaps, scale, blocks))
            blocks += nb

        for m in lin:
            w = m.weight
            ws = torch.empty_like(w, memory_format=torch.contiguous_format)
            bs = None
            add(0, w, ws, None, 0, 0, 0, m.scale, w.numel())
            if m.bias is not None:
                bs = torch.empty_like(m.bias)
                add(0, m.bias, bs, None, 0, 0, 0, m.lr_mul, m.bias.numel())
            m._live = (self, ws, bs)
            bufs += [ws, bs]
        for m in conv:
            w = m.weight
            cout, cin, k, _ = w.shape[-4:]
            wt = torch.empty((cin, k * k, cout), dtype=torch.float32, device=w.device)
            wsq = torch.empty((cout, cin), dtype=torch.float32, device=w.device)
            # the Winograd weight of every layer stylegan2.winograd_pays can name at some batch and plane (plain, wide);
            # a layer without one derives it per call (_native.wino_weight)
            u = None
            if WINOGRAD and k == 3 and not (m.upsample or m.downsample) and min(cin, cout) >= WINOGRAD_MIN_CHANNELS:
                u = torch.empty((16, cout, cin), dtype=torch.float32, device=w.device)
            add(1, w, wt, wsq, cout, cin, k * k, m.scale, 0, u)
            m._live = (self, wt, wsq)
            m._live_u = u
            bufs += [wt, wsq, u]
        table = np.array(rows, dtype=_ENTRY)
        dev = (lin[0].weight if lin else conv[0].weight).device
        self._table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        self._blocks, self._n, self._buffers, self._key = blocks, len(rows), bufs, key

    def refresh(self):
        """Re-derive every buffer from the parameters' current storage, on the current stream."""
        lin, conv = self._sources()
        if not lin and not conv:
            return False
        params = [m.weight for m in lin + conv] + [m.bias for m in lin if m.bias is not None]
        if any((not p.is_cuda) or p.dtype != torch.float32 or not p.is_contiguous() for p in params):
            return False
        key = tuple((p.data_ptr(), p.device.index) for p in params)
        if key != self._key:
            self._build(lin, conv, key)
        with _native.on_device(self._table) as stream:
            _native.check(_native.lib().fmgan_weight_refresh_f32(self._table.data_ptr(), self._n, self._blocks, stream),
                          'weight_refresh')
        return True

    def fresh(self):
        """Context: derived buffers are valid inside (refreshed on entry), ignored outside."""
        return _Fresh(self)


class _Fresh:
    def __init__(self, lw):
        self.lw = lw

    def __enter__(self):
        self.prev = self.lw.active
        if not self.prev:
            self.lw.active = self.lw.refresh()
        return self.lw

    def __exit__(self, *exc):
        self.lw.active = self.prev
        return False


def live(module):
    """(buffer, buffer) of `module` if it sits below a network whose inference forward is running right now."""
    lv = getattr(module, '_live', None)
    if lv is not None and lv[0].active and not torch.is_grad_enabled():
        return lv[1], lv[2]
    return None


def live_u(module):
    """The Winograd weight U [16, cout, cin] of a ModulatedConv2d from this forward's refresh, under live()'s condition; None
    outside a live forward and for a layer the table keeps no U for (the caller then derives it with _native.wino_weight)."""
    return getattr(module, '_live_u', None) if live(module) is not None else None


_SPLIT = weakref.WeakKeyDictionary()      # Conv2d module -> (key, image, built event, stream); not copied with the module


def split_conv_weight(conv, bracket='conv_weight_bf16x3'):
    """The three-piece bf16 image of `conv.weight` for _native.conv3x3s2_bf16x3 (built under the launch bracket `bracket`:
    conv_weight_to_bf16x3), kept per module and rebuilt only when the
    parameter's storage, device or autograd version changes: an optimizer step, `copy_` (load_state_dict) and any other
    in-place update of the PARAMETER bump `_version`; `p.data = ...` changes the storage.  (A write through `p.data` in
    place changes neither — see the module docstring; such an updater of an encoder calls drop_split_weight.  The
    encoder's inference weights come from load_state_dict.)"""
    w = conv.weight
    key = (w.data_ptr(), w._version, w.device, tuple(w.shape), tuple(w.stride()))
    kept = _SPLIT.get(conv)
    stream = torch.cuda.current_stream(w.device)
    if kept is None or kept[0] != key:
        img = _native.conv_weight_to_bf16x3(w, bracket)
        built = torch.cuda.Event()
        built.record(stream)
        kept = (key, img, built, stream)
        _SPLIT[conv] = kept
    elif kept[3] != stream:
        stream.wait_event(kept[2])          # built on another stream (the heads run on side streams)
    return kept[1]


def drop_split_weight(conv=None):
    """Forget the kept image of `conv` (None: of every module)."""
    if conv is None:
        _SPLIT.clear()
    else:
        _SPLIT.pop(conv, None)
