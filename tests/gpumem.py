"""Device and buffer helpers shared by the GPU tests (not a conftest: plain helpers, imported by name): the test device,
output buffers between guard words, and tensors that start 4 bytes past a 16-byte boundary."""
import numpy as np
import torch

GUARD = 64          # guard floats on each side of an output buffer
SENTINEL = 12345.5


def dev():
    return torch.device('cuda', 0)


def guarded(shape):
    """(buf, view): `view` has `shape` (an int n means (n,)) and is NaN-filled; `buf` holds it between GUARD sentinels."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev())
    buf[:GUARD] = SENTINEL
    buf[GUARD + n:] = SENTINEL
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def misaligned(t):
    """The same values in a view that starts one float into its storage (contiguous, 4 bytes off a 16-byte boundary)."""
    store = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = store[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def misaligned_nhwc(t):
    """The same values, NHWC-dense, starting 4 bytes past a 16-byte boundary."""
    n, c, h, w = t.shape
    store = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = store[1:].view(n, h, w, c).permute(0, 3, 1, 2)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.permute(0, 2, 3, 1).is_contiguous()
    return view
