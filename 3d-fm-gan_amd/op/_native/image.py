"""Image conversion, resizing, canvases and the image bank: csrc/image_io.hip, resize_plan.cpp, image_bank.hip."""
import ctypes

import torch

from .core import check, fp, launching, lib, on_device, ptr, require_f32_gpu, require_gpu


# ----------------------------------------------------------------------------- csrc/image_io.hip, csrc/resize_plan.cpp
def images_to_tensor(images, mean=0.5, std=0.5):
    """uint8 [B,H,W,3] (GPU) -> float32 [B,3,H,W] = ((images/255) - mean)/std: ToTensor + Normalize in one pass."""
    require_gpu(images, 'images')
    if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[-1] != 3:
        raise RuntimeError('images_to_tensor: expected a uint8 [B,H,W,3] tensor')
    x = images.contiguous()
    b, h, w, _ = x.shape
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=x.device)
    with on_device(x) as stream:
        check(lib().fmgan_images_to_tensor(ptr(x), ptr(out), b, h, w, float(mean), float(std), stream), 'images_to_tensor')
    return out


def resize_output_size(h, w, size):
    """torchvision Resize(int) rule: (out_h, out_w) for an [h, w] image (host logic, no GPU needed)."""
    oh, ow = ctypes.c_int(), ctypes.c_int()
    check(lib().fmgan_resize_output_size(int(h), int(w), int(size), ctypes.byref(oh), ctypes.byref(ow)), 'resize_output_size')
    return oh.value, ow.value


def resize_plan(in_h, in_w, out_h, out_w):
    """Pillow's bilinear coefficient tables for this size pair as a CPU int32 tensor (host logic, no GPU needed)."""
    n = lib().fmgan_resize_plan_ints(int(in_h), int(in_w), int(out_h), int(out_w))
    if n <= 0:
        raise RuntimeError('resize_plan: invalid sizes')
    plan = torch.empty(n, dtype=torch.int32)
    check(lib().fmgan_resize_plan(int(in_h), int(in_w), int(out_h), int(out_w), plan.data_ptr(), n), 'resize_plan')
    return plan


_PLANS = {}


def resize_images(images, out_h, out_w, to_tensor=False, mean=0.5, std=0.5):
    """uint8 [B,H,W,3] (GPU) -> PIL-exact bilinear resize.  to_tensor=False: uint8 [B,out_h,out_w,3];
    to_tensor=True: float32 [B,3,out_h,out_w] = ((v/255) - mean)/std (Resize + ToTensor + Normalize in one pass)."""
    require_gpu(images, 'images')
    if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[-1] != 3:
        raise RuntimeError('resize_images: expected a uint8 [B,H,W,3] tensor')
    x = images.contiguous()
    b, h, w, _ = x.shape
    key = (x.device, h, w, out_h, out_w)
    plan = _PLANS.get(key)
    if plan is None:
        plan = _PLANS[key] = resize_plan(h, w, out_h, out_w).to(x.device)
    if to_tensor:
        out = torch.empty((b, 3, out_h, out_w), dtype=torch.float32, device=x.device)
        o8, o32 = None, out
    else:
        out = torch.empty((b, out_h, out_w, 3), dtype=torch.uint8, device=x.device)
        o8, o32 = out, None
    with launching(x, 'resize', (b, h, w, out_h, out_w)) as stream:
        st = lib().fmgan_resize_bilinear_u8(ptr(x), ptr(plan), ptr(o8), ptr(o32), b, h, w, out_h, out_w, float(mean),
                                            float(std), stream)
    check(st, 'resize_bilinear_u8')
    return out


def tensor_to_images(tensor, cent=1.0, factor=255.0 / 2.0):
    """float32 [B,3,H,W] (GPU) -> uint8 [B,H,W,3] = uint8((clip(t,-1,1)+cent)*factor): tensor2im for the whole batch."""
    require_gpu(tensor, 'tensor')
    if tensor.dtype != torch.float32 or tensor.ndim != 4 or tensor.shape[1] != 3:
        raise RuntimeError('tensor_to_images: expected a float32 [B,3,H,W] tensor')
    x = tensor.contiguous()
    b, _, h, w = x.shape
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=x.device)
    with on_device(x) as stream:
        check(lib().fmgan_tensor_to_images(ptr(x), ptr(out), b, h, w, float(cent), float(factor), stream), 'tensor_to_images')
    return out


def tiles_to_canvas(src, canvas, slots, tile, cent=1.0, factor=255.0 / 2.0):
    """float32 [n,3,s,s] tiles into square slots of the uint8 canvas batch [C,H,W,3], in place, one launch
    (csrc/image_io.hip): slots int32 [n,3] ON src's DEVICE, one (canvas, y0, x0) per tile; s = tile, 2*tile or 4*tile (the
    tile is reduced by aten's bilinear rule).  The raw entry: op/canvas.py checks the layout on the host beforehand; the
    kernel skips a slot that does not lie inside its canvas.  Tensors of another dtype, device or layout are refused."""
    if src.ndim != 4 or src.shape[1] != 3 or src.shape[2] != src.shape[3] or canvas.ndim != 4 or canvas.shape[3] != 3 \
            or slots.ndim != 2 or tuple(slots.shape) != (src.shape[0], 3):
        raise ValueError(f'tiles_to_canvas: src {tuple(src.shape)}, canvas {tuple(canvas.shape)}, slots '
                         f'{tuple(slots.shape)}: expected [n, 3, s, s], [C, H, W, 3] and [n, 3]')
    require_f32_gpu('tiles_to_canvas', ((src, 'src'),))
    for t, name, dtype in ((canvas, 'canvas', torch.uint8), (slots, 'slots', torch.int32)):
        require_gpu(t, name)
        if t.dtype != dtype or not t.is_contiguous() or t.device != src.device:
            raise RuntimeError(f'tiles_to_canvas: {name} must be a contiguous {dtype} tensor on src\'s device, got '
                               f'{t.dtype} on {t.device} with strides {t.stride()}')
    n, _, s, _ = src.shape
    nc, ch, cw, _ = canvas.shape
    if n == 0:
        return canvas
    with launching(src, 'tiles_to_canvas', (n, s, int(tile), nc, ch, cw)) as stream:
        st = lib().fmgan_tiles_to_canvas(fp(src), ptr(canvas), ctypes.cast(slots.data_ptr(), ctypes.POINTER(ctypes.c_int)),
                                         n, s, int(tile), nc, ch, cw, float(cent), float(factor), stream)
    check(st, 'tiles_to_canvas')
    return canvas


# ----------------------------------------------------------------------------- csrc/image_bank.hip
BANK_GATHER_BANKS, BANK_GATHER_GROUPS = 4, 8      # csrc/image_bank.hip: BG_MAX_BANKS, BG_MAX_GROUPS


def bank_gather(banks, index_a, index_b, offset, members, stride, groups, mean=0.5, std=0.5, out=None,
                pixels_per_lane=0):
    """out[s] = ((bank[k_s][i_s] / 255) - mean) / std in one launch (csrc/image_bank.hip): `banks` up to 4 uint8
    [N_k,H,W,3] GPU tensors of one H x W (contiguous; a view into a larger storage is fine), index_a / index_b int32 GPU
    tensors (index_b may be None), `groups` a sequence of (bank, source, swap, mul, add); returns float32
    [len(groups) * members, 3, H, W], group after group.  The raw entry: op/image_bank.py checks index ranges and the
    pairing on the host beforehand; the kernel skips a slot whose bank, position or image index is out of range.
    Tensors of another dtype, device or layout are refused.  members == 0: an empty tensor, no launch."""
    banks = list(banks)
    groups = [tuple(int(v) for v in g) for g in groups]
    if not 1 <= len(banks) <= BANK_GATHER_BANKS or not 1 <= len(groups) <= BANK_GATHER_GROUPS \
            or any(len(g) != 5 for g in groups):
        raise ValueError(f'bank_gather: {len(banks)} banks and {len(groups)} groups: 1..{BANK_GATHER_BANKS} banks and '
                         f'1..{BANK_GATHER_GROUPS} groups of (bank, source, swap, mul, add)')
    first = banks[0]
    for k, t in enumerate(banks):
        require_gpu(t, f'banks[{k}]')
        if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[3] != 3 or not t.is_contiguous() or t.device != first.device:
            raise RuntimeError(f'bank_gather: banks[{k}] must be a contiguous uint8 [N,H,W,3] tensor on banks[0]\'s '
                               f'device, got {t.dtype} {tuple(t.shape)} on {t.device} with strides {t.stride()}')
        if tuple(t.shape[1:3]) != tuple(first.shape[1:3]):
            raise ValueError(f'bank_gather: banks[{k}] holds {tuple(t.shape[1:3])} images, banks[0] '
                             f'{tuple(first.shape[1:3])}')
    for t, name in ((index_a, 'index_a'), (index_b, 'index_b')):
        if t is None and name == 'index_b':
            continue
        require_gpu(t, name)
        if t.dtype != torch.int32 or t.ndim != 1 or not t.is_contiguous() or t.device != first.device:
            raise RuntimeError(f'bank_gather: {name} must be a contiguous int32 vector on the banks\' device')
    h, w = int(first.shape[1]), int(first.shape[2])
    members, n = int(members), int(members) * len(groups)
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=first.device)
    else:
        require_f32_gpu('bank_gather', ((out, 'out'),))
        if tuple(out.shape) != (n, 3, h, w) or out.device != first.device:
            raise ValueError(f'bank_gather: out {tuple(out.shape)} on {out.device}, expected {(n, 3, h, w)} on '
                             f'{first.device}')
    if n == 0:
        return out
    ptrs = [ptr(t) for t in banks] + [None] * (BANK_GATHER_BANKS - len(banks))
    counts = [int(t.shape[0]) for t in banks] + [0] * (BANK_GATHER_BANKS - len(banks))
    table = (ctypes.c_int * (5 * len(groups)))(*[v for g in groups for v in g])
    with launching(first, 'bank_gather', (n, h, w, len(groups), int(stride))) as stream:
        st = lib().fmgan_bank_gather(*ptrs, *counts, h, w, ptr(index_a), int(index_a.numel()), ptr(index_b),
                                     0 if index_b is None else int(index_b.numel()), int(offset), members, int(stride),
                                     table, len(groups), fp(out), float(mean), float(std), int(pixels_per_lane), stream)
    check(st, 'bank_gather')
    return out
