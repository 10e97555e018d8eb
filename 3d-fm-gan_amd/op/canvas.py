"""Many float images into one uint8 picture on the GPU (csrc/image_io.hip, fmgan_tiles_to_canvas): the last step of
the sample sheets and video triptychs of Evaluation/visual_eval.py.  One launch per group of equally sized tiles, no
intermediate image, and the sheet leaves the device in one copy.  The layout is host arithmetic; it is checked here, on
the host, before anything reaches the kernel."""
import numpy as np
import torch

from . import _native


def sheet_layout(n_rows, n_cols, tile, gap=0, margin=0):
    """(canvas_h, canvas_w, yx): a grid of n_rows x n_cols square tiles of side `tile`, `gap` pixels between neighbours
    and `margin` around the grid; yx [n_rows * n_cols, 2] int64 holds each tile's top-left corner, row by row.  Host
    integers only."""
    n_rows, n_cols, tile, gap, margin = (int(v) for v in (n_rows, n_cols, tile, gap, margin))
    if n_rows < 1 or n_cols < 1 or tile < 1 or gap < 0 or margin < 0:
        raise ValueError(f'sheet_layout: {n_rows} x {n_cols} tiles of {tile}, gap {gap}, margin {margin}: rows, columns '
                         f'and tile must be positive, gap and margin non-negative')
    canvas_h = 2 * margin + n_rows * tile + (n_rows - 1) * gap
    canvas_w = 2 * margin + n_cols * tile + (n_cols - 1) * gap
    rows, cols = np.divmod(np.arange(n_rows * n_cols, dtype=np.int64), n_cols)
    yx = np.stack([margin + rows * (tile + gap), margin + cols * (tile + gap)], 1)
    return canvas_h, canvas_w, yx


def check_slots(slots, n, tile, n_canvas, canvas_h, canvas_w):
    """`slots` as an int32 [n, 3] host array of (canvas, y0, x0) — (y0, x0) rows name canvas 0 — after the layout checks:
    one slot per tile, every slot wholly inside its canvas, no two slots of a canvas sharing a pixel (ValueError)."""
    s = np.asarray(slots)
    if s.size == 0:
        s = np.zeros((0, 3), np.int64)
    if s.ndim != 2 or s.shape[1] not in (2, 3) or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f'tiles_to_canvas: slots of shape {s.shape} and dtype {s.dtype}: expected integer rows of '
                         f'(canvas, y0, x0) or (y0, x0)')
    s = s.astype(np.int64)
    if s.shape[1] == 2:
        s = np.concatenate([np.zeros((s.shape[0], 1), np.int64), s], 1)
    if s.shape[0] != n:
        raise ValueError(f'tiles_to_canvas: {s.shape[0]} slots for {n} tiles')
    c, y, x = s[:, 0], s[:, 1], s[:, 2]
    bad = (c < 0) | (c >= n_canvas) | (y < 0) | (x < 0) | (y + tile > canvas_h) | (x + tile > canvas_w)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f'tiles_to_canvas: slot {k} = (canvas {c[k]}, y0 {y[k]}, x0 {x[k]}) of side {tile} does not lie '
                         f'inside a batch of {n_canvas} canvases of {canvas_h} x {canvas_w}')
    # two squares of one side overlap iff both corner distances are below the side; sorted by (canvas, y0) a slot can
    # only meet the slots that follow it up to the first one `tile` rows further down
    order = np.lexsort((x, y, c))
    cs, ys, xs = c[order], y[order], x[order]
    for a in range(n):
        b = a + 1
        while b < n and cs[b] == cs[a] and ys[b] - ys[a] < tile:
            if abs(xs[b] - xs[a]) < tile:
                raise ValueError(f'tiles_to_canvas: slots {int(order[a])} and {int(order[b])} overlap on canvas '
                                 f'{int(cs[a])}: ({ys[a]}, {xs[a]}) and ({ys[b]}, {xs[b]}) at side {tile}')
            b += 1
    return np.ascontiguousarray(s, dtype=np.int32)


def tiles_to_canvas(src, canvas, slots, tile, cent=1., factor=255. / 2.):
    """src float32 [n, 3, s, s] on the GPU into `canvas`, uint8 [H, W, 3] or [C, H, W, 3] on the same device, in place:
    tile i goes to the square of side `tile` whose top-left corner slots[i] = (canvas, y0, x0) or (y0, x0) names (a host
    list or array), as uint8((clip(v, -1, 1) + cent) * factor) — tensor2im's value — of the pixel (s == tile) or of its
    bilinear reduction (s == 2 * tile, 4 * tile; F.interpolate at align_corners=False).  Bytes outside the tiles keep
    their value.  Slots outside the canvas, overlapping slots and any other ratio raise ValueError before anything is
    launched; CPU tensors and other dtypes raise RuntimeError (no fallback).  The slots are uploaded once, without a
    synchronisation, and one kernel is launched.  Returns `canvas`."""
    if not torch.is_tensor(canvas) or canvas.ndim not in (3, 4) or canvas.shape[-1] != 3:
        raise ValueError(f'tiles_to_canvas: canvas {tuple(canvas.shape)}: expected uint8 [H, W, 3] or [C, H, W, 3]')
    if src.ndim != 4 or src.shape[1] != 3 or src.shape[2] != src.shape[3]:
        raise ValueError(f'tiles_to_canvas: src {tuple(src.shape)}: expected [n, 3, s, s]')
    tile = int(tile)
    n, s = src.shape[0], src.shape[2]
    if tile < 1 or s not in (tile, 2 * tile, 4 * tile):
        raise ValueError(f'tiles_to_canvas: tiles of {s} x {s} into slots of side {tile}: the ratio must be 1, 2 or 4')
    batch = canvas if canvas.ndim == 4 else canvas.unsqueeze(0)
    host = check_slots(slots, n, tile, batch.shape[0], batch.shape[1], batch.shape[2])
    _native.require_f32_gpu('tiles_to_canvas', ((src, 'src'),))
    _native.require_gpu(canvas, 'canvas')
    if n == 0:
        return canvas
    dev_slots = torch.from_numpy(host).to(src.device, non_blocking=True)
    _native.tiles_to_canvas(src, batch, dev_slots, tile, cent, factor)
    return canvas
