"""GPU tests of fmgan_tiles_to_canvas through op/canvas.py: float tiles into slots of guarded uint8 canvases, at the
smallest shapes at which the kernel can go wrong — tiles of 4 (one full unit per row, the vector form), 6 and 10 (a
ragged last unit, the bounded form), every reduction, row pitches that are and are not a multiple of 4 bytes, odd and even
x0, slots in permuted order, a partly filled last row, one canvas and a batch of two."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpumem import dev, guarded, guards_intact
from launches import observed

pytestmark = pytest.mark.gpu

LAYOUTS = [(1, 1, 23), (1, 1, 32), (5, 1, 23), (5, 2, 32)]       # (tiles, canvases, canvas_w)


def _slots(n, n_canvas, canvas_w, tile):
    """(canvas_h, slots [n, 3]): tiles one pixel apart from x = 1 on (so x0 is odd, even, odd, ...), dealt over the
    canvases in turn, then permuted so that tile i does not sit at position i."""
    per_row = (canvas_w - 1) // (tile + 1)
    assert per_row >= 2 and 1 + per_row * (tile + 1) - 1 <= canvas_w
    per_canvas = -(-n // n_canvas)
    rows = -(-per_canvas // per_row)
    canvas_h = 2 + rows * (tile + 1)
    slots = []
    for k in range(n):
        c, q = k % n_canvas, k // n_canvas
        slots.append((c, 2 + (q // per_row) * (tile + 1), 1 + (q % per_row) * (tile + 1)))
    assert {s[2] & 1 for s in slots} == ({0, 1} if n > 1 else {1})
    order = np.random.Generator(np.random.Philox(key=n * 131 + tile)).permutation(n)
    return canvas_h, [slots[j] for j in order]


def _src(n, s, f, tag):
    """U(-1.5, 1.5) so that the clamp acts, with exact -1, 0 and 1 scattered and as whole f x f cells."""
    g = torch.Generator().manual_seed(1000 * s + 10 * n + f)
    x = torch.rand((n, 3, s, s), generator=g) * 3.0 - 1.5
    flat = x.view(-1)
    flat[::7], flat[3::11], flat[5::13] = 1.0, -1.0, 0.0
    x[0, 0, :f, :f], x[0, 1, :f, :f], x[0, 2, :f, :f] = 1.0, -1.0, 0.0
    assert float(x.max()) > 1.0 and float(x.min()) < -1.0
    return x.to(dev())


def _canvas(n_canvas, h, w):
    """(guard buffer, every interior byte, the canvas [C,H,W,3] or [H,W,3] inside it) pre-filled with a byte pattern."""
    nbytes = n_canvas * h * w * 3
    buf, words = guarded(-(-nbytes // 4))
    inner = words.view(torch.uint8)
    inner.copy_((torch.arange(inner.numel(), device=dev()) % 251).to(torch.uint8))
    canvas = inner[:nbytes].view(n_canvas, h, w, 3)
    return buf, inner, (canvas if n_canvas > 1 else canvas[0])


def _reduced(src, f):
    """The stated formula in torch on the device, with the kernel's association: 0.5*a + 0.5*b per pair, columns first."""
    if f == 1:
        return src
    o = f // 2 - 1
    a, b = src[:, :, o::f, o::f], src[:, :, o::f, o + 1::f]
    c, d = src[:, :, o + 1::f, o::f], src[:, :, o + 1::f, o + 1::f]
    top, bottom = 0.5 * a + 0.5 * b, 0.5 * c + 0.5 * d
    return (0.5 * top + 0.5 * bottom).contiguous()


def _placed(before, tiles_u8, slots, tile):
    ref = before.clone()
    batch = ref if ref.ndim == 4 else ref.unsqueeze(0)
    for i, (c, y0, x0) in enumerate(slots):
        batch[c, y0:y0 + tile, x0:x0 + tile] = tiles_u8[i]
    return ref


@pytest.mark.parametrize('layout', LAYOUTS, ids=lambda l: 'n%d-c%d-w%d' % l)
@pytest.mark.parametrize('f', [1, 2, 4])
@pytest.mark.parametrize('tile', [4, 6, 10])
def test_tiles_to_canvas(tile, f, layout):
    from Evaluation.visual_eval import tensor2im_batch
    from op.canvas import tiles_to_canvas
    n, n_canvas, canvas_w = layout
    canvas_h, slots = _slots(n, n_canvas, canvas_w, tile)
    src = _src(n, f * tile, f, 'canvas')
    buf, inner, canvas = _canvas(n_canvas, canvas_h, canvas_w)
    before, inner_before = canvas.clone(), inner.clone()
    given = slots if n_canvas > 1 else [s[1:] for s in slots]          # (y0, x0) rows name the single canvas
    with observed() as rec:
        out = tiles_to_canvas(src, canvas, given, tile)
    assert out is canvas and rec.names == ['tiles_to_canvas']           # exactly one launch
    assert guards_intact(buf)
    nbytes = canvas.numel()
    assert torch.equal(inner[nbytes:], inner_before[nbytes:])
    # f = 1: tensor2im_batch placed by slicing; f = 2, 4: the formula, bit for bit; everything else keeps the pattern
    v = _reduced(src, f)
    assert tuple(v.shape) == (n, 3, tile, tile)
    want = _placed(before, tensor2im_batch(v), slots, tile)
    assert torch.equal(canvas, want)
    assert not torch.equal(canvas, before)
    if f == 1:
        return
    # against aten's own bilinear reduction: a byte may differ, by exactly 1, only where (clip(v)+1)*127.5 lies within
    # 127.5 * 2^-22 of an integer (two fp32 roundings at |v| <= 1 between the two associations)
    aten = tensor2im_batch(F.interpolate(src, size=tile, mode='bilinear', align_corners=False))
    ours = tensor2im_batch(v)
    x = (v.double().clamp(-1, 1) + 1.0) * 127.5
    near = (x - x.round()).abs() <= 127.5 * 2.0 ** -22
    diff = (ours.int() - aten.int()).abs().permute(0, 3, 1, 2)
    assert int(diff.max()) <= 1
    assert not bool((diff.bool() & ~near).any())


def test_tiles_to_canvas_exact_values_and_clamp():
    """-1, 0, 1 and values beyond the clamp, as whole tiles at every reduction: 0, 127, 255 (tensor2im's truncation)."""
    from op.canvas import tiles_to_canvas
    for f in (1, 2, 4):
        vals = torch.tensor([-1.0, 0.0, 1.0, -1.5, 1.5], device=dev())
        src = vals.view(5, 1, 1, 1).expand(5, 3, 4 * f, 4 * f).contiguous()
        canvas = torch.full((5, 4, 23, 3), 9, dtype=torch.uint8, device=dev())
        tiles_to_canvas(src, canvas, [(k, 0, 2 * k + 1) for k in range(5)], 4)
        for k, b in enumerate((0, 127, 255, 0, 255)):
            assert bool((canvas[k, :, 2 * k + 1:2 * k + 5] == b).all()), (f, k)
            assert bool((canvas[k, :, :2 * k + 1] == 9).all()) and bool((canvas[k, :, 2 * k + 5:] == 9).all())


def test_layout_is_refused_on_the_host_before_any_launch():
    from op.canvas import tiles_to_canvas
    src = torch.zeros((2, 3, 4, 4), device=dev())
    canvas = torch.zeros((8, 23, 3), dtype=torch.uint8, device=dev())
    with observed() as rec:
        for slots in ([(0, 0), (5, 0)], [(0, 20), (4, 0)], [(-1, 0), (4, 0)], [(1, 0, 0), (0, 4, 0)],       # outside
                      [(0, 0), (3, 3)], [(0, 0), (0, 0)],                                                   # overlapping
                      [(0, 0)], [(0, 0, 0, 0), (0, 0, 4, 0)]):                                              # malformed
            with pytest.raises(ValueError):
                tiles_to_canvas(src, canvas, slots, 4)
        with pytest.raises(ValueError):
            tiles_to_canvas(torch.zeros((1, 3, 12, 12), device=dev()), canvas, [(0, 0)], 4)                 # ratio 3
        with pytest.raises(ValueError):
            tiles_to_canvas(src, canvas[..., :2], [(0, 0), (4, 0)], 4)
    assert rec.seen == [] and not bool(canvas.any())


def test_other_devices_and_dtypes_raise():
    from op import _native
    from op.canvas import tiles_to_canvas
    src = torch.zeros((1, 3, 4, 4), device=dev())
    canvas = torch.zeros((8, 23, 3), dtype=torch.uint8, device=dev())
    with observed() as rec:
        with pytest.raises(RuntimeError):
            tiles_to_canvas(src.cpu(), canvas, [(0, 0)], 4)
        with pytest.raises(RuntimeError):
            tiles_to_canvas(src.double(), canvas, [(0, 0)], 4)
        with pytest.raises(RuntimeError):
            tiles_to_canvas(src, canvas.cpu(), [(0, 0)], 4)
        with pytest.raises(RuntimeError):
            tiles_to_canvas(src, canvas.float(), [(0, 0)], 4)
        slots = torch.zeros((1, 3), dtype=torch.int32, device=dev())
        with pytest.raises(RuntimeError):
            _native.tiles_to_canvas(src, canvas.unsqueeze(0), slots.cpu(), 4)
        with pytest.raises(RuntimeError):
            _native.tiles_to_canvas(src, canvas.unsqueeze(0), slots.long(), 4)
    assert rec.seen == []


def test_no_tiles_returns_at_once():
    from op.canvas import tiles_to_canvas
    canvas = torch.full((8, 23, 3), 7, dtype=torch.uint8, device=dev())
    with observed() as rec:
        assert tiles_to_canvas(torch.zeros((0, 3, 8, 8), device=dev()), canvas, [], 4) is canvas
    assert rec.seen == [] and bool((canvas == 7).all())
