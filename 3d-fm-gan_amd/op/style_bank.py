"""Styles and demodulation coefficients of a whole Generator in two launches (csrc/style_bank.hip).

With co-modulation inputs that are complete before the synthesis network starts (re-animation: W+ of the photo is
cached, W of the render frames is known) no layer's style depends on an activation, so the per-layer
`fmgan_equal_linear_f32` / `fmgan_modconv_demod_wsq_f32` launches and the `W * W+[:, i]` multiplies leave the critical
path: a device-side table with one entry per modulated conv (conv1, to_rgb1, every convs[i], every to_rgbs[i]) points
at the layer's refreshed `weight*scale` / `bias*lr_mul` / `sum_tap W^2` buffers (op/live_weights.py) and at its slot
in two flat output buffers.  The table holds raw pointers of the LiveWeights buffers, so it is rebuilt whenever
LiveWeights rebuilds (recognised by the identity of its device table, which every rebuild replaces), a deep copy starts
without one, and it is valid only inside the Generator's inference forward, after the weight refresh.

The concatenating co-modulation modes of the 2-encoder scheme ('Concatenation', 'Tensor Transform') modulate with
x = [V | W+[:, col]] over a [cin, Dv + Dw] matrix: `run_concat` is the same table walked by fmgan_style_bank_concat_f32
(the concatenation is never materialised), then the same demodulation launch.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native
from .live_weights import live


class Modulation(NamedTuple):
    """A layer's modulation, already computed: what a StyledConv / ToRGB accepts as `style` in place of a latent column."""
    style: torch.Tensor             # [B, cin]
    demod: Optional[torch.Tensor]   # [B, cout]; None where the layer does not demodulate


def sliced_columns(sliced_layer, n_latent, n_styles):
    """The co-modulated columns of a W+ with n_styles columns: `sliced_layer`, or every column of the Generator for None,
    minus what W+ does not have."""
    return frozenset(i for i in (range(n_latent) if sliced_layer is None else sliced_layer) if 0 <= i < n_styles)


def comod_column(w, wplus_i, i, sliced):
    """Latent column i of the multiplicative co-modulation: W * W+[:, i] where sliced, W elsewhere."""
    return w * wplus_i if i in sliced else w


def concat_column(v, wplus_i):
    """Latent column of the concatenating co-modulation: [V | W+[:, i]] ([T, Dv + Dw]; W+ of one photo serves T frames)."""
    if wplus_i.shape[0] != v.shape[0]:
        wplus_i = wplus_i.expand(v.shape[0], -1)
    return torch.cat([v, wplus_i], 1)

_ENTRY = np.dtype([('ws', '<u8'), ('bs', '<u8'), ('wsq', '<u8'), ('style_off', '<i8'), ('demod_off', '<i8'),
                   ('col', '<i4'), ('sliced', '<i4'), ('n_styles', '<i4'), ('cin', '<i4'), ('cout', '<i4'),
                   ('demodulate', '<i4'), ('scale', '<f4'), ('eps', '<f4')])


def _check_layout():
    if _native.lib().fmgan_style_bank_entry_bytes() != _ENTRY.itemsize:
        raise RuntimeError('fmgan_style_bank_entry layout mismatch between libfmgan_hip.so and op/style_bank.py')


class Table:
    """Device table + slot layout for a list of layers, each a dict(ws, bs, wsq, col, sliced, cout, scale, eps,
    demodulate) of f32 GPU tensors (bs / wsq may be None) and scalars; cin is ws.shape[0]."""

    def __init__(self, layers, n_styles):
        _check_layout()
        rows, self.style_slots, self.demod_slots = [], [], []
        s_off = d_off = 0
        for l in layers:
            cin, cout = int(l['ws'].shape[0]), int(l['cout'])
            demod = bool(l['demodulate']) and l['wsq'] is not None
            if l['sliced'] and not 0 <= int(l['col']) < n_styles:
                raise RuntimeError(f"style_bank: sliced column {l['col']} outside W+'s {n_styles} columns")
            if l['ws'].dim() != 2 or l['ws'].shape[1] != layers[0]['ws'].shape[1] or not l['ws'].is_contiguous() or (l['wsq'] is not None and (
                    tuple(l['wsq'].shape) != (cout, cin) or not l['wsq'].is_contiguous())) or (
                    l['bs'] is not None and l['bs'].numel() != cin):
                raise RuntimeError('style_bank: ws [cin,D], bs [cin], wsq [cout,cin], contiguous')
            rows.append((_native.fp(l['ws']), _native.fp(l['bs']) or 0, _native.fp(l['wsq']) or 0, s_off, d_off,
                         int(l['col']), int(bool(l['sliced'])), int(n_styles), cin, cout, int(demod), l['scale'], l['eps']))
            self.style_slots.append((s_off, cin))
            self.demod_slots.append((d_off, cout) if demod else None)
            s_off += cin
            d_off += cout if demod else 0
        self.n, self.n_styles = len(rows), int(n_styles)
        self.cols = [int(l['col']) for l in layers]
        self.style_floats, self.demod_floats = s_off, d_off
        self.style_dim = int(layers[0]['ws'].shape[1])
        self.device = layers[0]['ws'].device
        self.dev = torch.from_numpy(np.array(rows, dtype=_ENTRY).view(np.uint8).copy()).to(self.device)

    def buffers(self, batch):
        """(flat styles, flat demod) for `batch` samples (demod holds one spare float when nothing is demodulated)."""
        return (torch.empty(batch * self.style_floats, dtype=torch.float32, device=self.device),
                torch.empty(max(1, batch * self.demod_floats), dtype=torch.float32, device=self.device))

    def run(self, w, wplus, styles, demod):
        """The two launches on the current stream."""
        if (wplus.dim() != 3 or wplus.shape[1] != self.n_styles or w.shape[1] != self.style_dim
                or styles.numel() < w.shape[0] * self.style_floats or demod.numel() < w.shape[0] * self.demod_floats):
            raise RuntimeError('style_bank: buffers, style_dim or W+ columns do not match the table')
        _native.style_bank(self.dev, self.n, w, wplus, styles)
        if self.demod_floats:
            _native.demod_bank(self.dev, self.n, styles, w.shape[0], demod)

    def run_concat(self, v, wplus, styles, demod):
        """The two launches of the concatenating co-modulation, x = [v | wplus[:, col]], on the current stream.  Every
        entry's column is read (the `sliced` flags are not), so every one must be a column of W+."""
        if (v.dim() != 2 or wplus.dim() != 3 or wplus.shape[1] != self.n_styles
                or v.shape[1] + wplus.shape[2] != self.style_dim or wplus.shape[0] not in (1, v.shape[0])
                or styles.numel() < v.shape[0] * self.style_floats or demod.numel() < v.shape[0] * self.demod_floats):
            raise RuntimeError('style_bank: buffers, Dv + Dw = style_dim, W+ columns or batch do not match the table')
        if not all(0 <= c < self.n_styles for c in self.cols):
            raise RuntimeError(f"style_bank: a concatenated column lies outside W+'s {self.n_styles} columns")
        _native.style_bank_concat(self.dev, self.n, v, wplus, styles)
        if self.demod_floats:
            _native.demod_bank(self.dev, self.n, styles, v.shape[0], demod)

    def views(self, batch, styles, demod):
        """Per-layer Modulation([batch,cin] style, [batch,cout] demod or None): views into the flat buffers."""
        out = []
        for (so, cin), ds in zip(self.style_slots, self.demod_slots):
            s = styles[batch * so:batch * (so + cin)].view(batch, cin)
            d = None if ds is None else demod[batch * ds[0]:batch * (ds[0] + ds[1])].view(batch, ds[1])
            out.append(Modulation(s, d))
        return out


class StyleBank:
    """The bank of one Generator: tables per (sliced columns, n_styles) — the concatenating form's under a key of its
    own — and output buffers per batch size."""

    def __init__(self, generator):
        self.root = generator
        self._source = None     # the LiveWeights device table our pointers were taken under (kept alive: identity is the key)
        self._tables = {}
        self._buffers = {}

    def __deepcopy__(self, memo):
        import copy
        new = StyleBank.__new__(StyleBank)
        memo[id(self)] = new
        new.__init__(copy.deepcopy(self.root, memo))
        return new

    def layers(self):
        """(ModulatedConv2d, latent column) of every modulated conv, in forward order."""
        g = self.root
        out = [(g.conv1.conv, 0), (g.to_rgb1.conv, 1)]
        for blk, to_rgb in enumerate(g.to_rgbs):
            i = 1 + 2 * blk
            out += [(g.convs[2 * blk].conv, i), (g.convs[2 * blk + 1].conv, i + 1), (to_rgb.conv, i + 2)]
        return out

    def _table(self, sliced, n_styles):
        lw = self.root._live_weights
        if lw is None or not lw.active:
            raise RuntimeError('StyleBank is valid only inside its Generator\'s inference forward (after the weight refresh)')
        if lw._table is not self._source:   # LiveWeights rebuilt its buffers: every pointer of every table is stale.  Its
            # pointer key would miss a rebuild A -> B -> A between two of our forwards; a rebuild always makes a new table.
            self._source, self._tables, self._buffers = lw._table, {}, {}
        tk = (sliced, n_styles)      # sliced: a frozenset of columns, or 'concat' (every column, the flags unused)
        if tk not in self._tables:
            rows = []
            for conv, col in self.layers():
                ws, bs = live(conv.modulation)
                lv = live(conv) if conv.kernel_size == 3 else None
                rows.append(dict(ws=ws, bs=bs, wsq=lv[1] if lv else None, col=col,
                                 sliced=sliced != 'concat' and col in sliced,
                                 cout=conv.out_channel, scale=conv.scale, eps=conv.eps, demodulate=conv.demodulate))
                if conv.demodulate and lv is None:
                    raise RuntimeError('style_bank: a demodulated layer without refreshed weight squares')
            self._tables[tk] = Table(rows, n_styles)
        return self._tables[tk]

    def run(self, w, wplus, sliced):
        """{ModulatedConv2d: Modulation(style [T,cin], demod [T,cout] or None)} for W [T,D], W+ [P,n_styles,D], P in {1,T}, and
        the set of co-modulated columns."""
        table = self._table(frozenset(sliced), int(wplus.shape[1]))
        batch = int(w.shape[0])
        if batch not in self._buffers:
            self._buffers[batch] = table.buffers(batch)
        styles, demod = self._buffers[batch]
        table.run(w, wplus, styles, demod)
        return {conv: v for (conv, _), v in zip(self.layers(), table.views(batch, styles, demod))}

    def run_concat(self, v, wplus):
        """The same mapping for the concatenating co-modulation: V [T,Dv], W+ [P,n_styles,Dw], Dv + Dw = style_dim."""
        table = self._table('concat', int(wplus.shape[1]))
        batch = int(v.shape[0])
        if batch not in self._buffers:
            self._buffers[batch] = table.buffers(batch)
        styles, demod = self._buffers[batch]
        table.run_concat(v, wplus, styles, demod)
        return {conv: m for (conv, _), m in zip(self.layers(), table.views(batch, styles, demod))}
