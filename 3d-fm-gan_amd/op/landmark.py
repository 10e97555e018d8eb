"""Tensor stages around the landmark networks (reference Util/landmark_util.py, Util/training_util.py:206-222): what the
reference wraps around the face detector and the alignment network, without the networks.

    face_crop(img, box, r)           Get_HeatMap_PyTorch's scaling to [0, 255], Crop_PyTorch for every sample and the
                                     division by 255: img [N, 3, H, W] in [-1, 1], box [N, 4] int32 (ux, uy, bx, by: the
                                     inverse transform of (1, 1) and (r, r)) -> [N, 3, r, r] in [0, 1], differentiable
                                     with respect to img
    detector_input(img)              ((img + 1) * 255 / 2).flip(1) - (104, 117, 123): the detector's input, no gradient
    heatmap_distance(a, b)           [N] sums of (a - b)^2 over everything but the batch axis, differentiable in both
    landmark_decode(hm, c, s)        _get_preds_fromhm_torch: (preds, preds_orig), each [B, C, 2], no gradient

On the MI355X kernels (csrc/landmark.hip) each stage is one launch per direction for the whole batch, float32 and
bit-reproducible (the distance: fixed-order partials added here in float64; the crop's backward: a gather in fixed order).
The reference builds each crop on the host (one device-to-host copy, one interpolate and one copy back per image) and
decodes with two host synchronisations and four scalar reads per map; here nothing synchronises: the boxes travel to
the kernel as a small int32 tensor and the upstream gradient of the distance as a device tensor.

Every stage has a composite from aten ops (`*_composite`: any device, dtype and size, differentiable to any order; the
CPU path) and a predicate (`*_serves`: float32 contiguous CUDA tensors, autocast off, and the stage's own sizes).
LANDMARK_FUSE = False (or FMGAN_NO_LANDMARK_FUSE=1) keeps the composites everywhere.  First order only on the kernels,
hence once_differentiable: a double backward raises.  The crop's tap positions follow aten's fp32 rule
(include/fmgan_hip.h); its association of the products is fixed and may differ from aten's in the last bits.
"""
import os

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from ._native import amp_fwd as _amp_fwd, amp_bwd as _amp_bwd

LANDMARK_FUSE = os.environ.get('FMGAN_NO_LANDMARK_FUSE', '0') != '1'
HEATMAP_SIZE = _native.HEATMAP_SIZE
DETECTOR_MEAN = (104.0, 117.0, 123.0)


def _fuse(fuse):
    return LANDMARK_FUSE if fuse is None else bool(fuse)


def _f32_cuda(*tensors):
    first = tensors[0]
    return first.is_cuda and not torch.is_autocast_enabled() and all(
        t.dtype == torch.float32 and t.device == first.device and t.is_contiguous() for t in tensors)


def box_tensor(box, n):
    """The crop boxes as an int32 [n, 4] tensor (where they are: host lists become a host tensor)."""
    box = torch.as_tensor(box)
    if tuple(box.shape) != (n, 4) or box.is_floating_point():
        raise ValueError(f'face_crop: box {tuple(box.shape)} {box.dtype}: expected [{n}, 4] integers (ux, uy, bx, by)')
    return box.to(torch.int32)


# ----------------------------------------------------------------------------- face crop
class FaceCropFunction(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, img, box, r):
        out = _native.face_crop_fwd(img, box, r)
        if out is None:
            raise RuntimeError(f'face_crop: no kernel for images {tuple(img.shape)} at {r} (ask face_crop_serves first)')
        ctx.save_for_backward(box)
        ctx.size = tuple(img.shape[2:])
        return out

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, grad_out):
        box, = ctx.saved_tensors
        grad_img = _native.face_crop_bwd(grad_out.to(torch.float32).contiguous(), box, *ctx.size)
        if grad_img is None:
            raise RuntimeError(f'face_crop: no backward kernel for crops {tuple(grad_out.shape)}')
        return grad_img, None, None


def crop_canvas(scaled, box, r):
    """Crop_PyTorch for every sample of `scaled` [N, C, H, W] from aten ops: a zero canvas of the box's size, the image's
    part of it copied in, F.interpolate to r x r.  Keeps the image's range; the canvas is on the image's device."""
    n, c, h, w = scaled.shape
    boxes = box_tensor(box, n).tolist()
    crops = []
    for i, (ux, uy, bx, by) in enumerate(boxes):
        hc, wc = by - uy, bx - ux
        if hc < 1 or wc < 1:
            raise ValueError(f'face_crop: box {boxes[i]} of sample {i} is empty')
        canvas = scaled.new_zeros((1, c, hc, wc))
        y0, y1, x0, x1 = max(uy, 0), min(by, h), max(ux, 0), min(bx, w)
        if y1 > y0 and x1 > x0:
            canvas[..., y0 - uy:y1 - uy, x0 - ux:x1 - ux] = scaled[i:i + 1, :, y0:y1, x0:x1]
        crops.append(F.interpolate(canvas, (r, r), mode='bilinear', align_corners=False))
    return torch.cat(crops)


def face_crop_composite(img, box, r):
    """The crop from aten ops, operation for operation the reference's: the scaling to [0, 255], crop_canvas, / 255.  Any
    device and dtype."""
    return crop_canvas((img + 1) * 255 / 2, box, r) / 255.0


def face_crop_serves(img, r):
    """Do the kernels take this call (host logic, nothing runs)?"""
    if not (torch.is_tensor(img) and img.ndim == 4 and img.shape[1] == 3 and _f32_cuda(img)):
        return False
    return _native.face_crop_serves(img.shape[0], img.shape[2], img.shape[3], int(r))


def face_crop(img, box, r=256, fuse=None):
    """[N, 3, r, r] crops in [0, 1] of img [N, 3, H, W] in [-1, 1]: the kernels where face_crop_serves() (and `fuse`), the
    composite elsewhere.  box: [N, 4] integers (ux, uy, bx, by), a host list or tensor (copied to the device without a
    synchronisation) or a device tensor; every box must be non-empty (checked where the box is on the host)."""
    if _fuse(fuse) and face_crop_serves(img, r):
        b = box_tensor(box, img.shape[0])
        if not b.is_cuda:
            sides = torch.stack((b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]))
            if bool((sides < 1).any()) or bool((sides > 1 << 24).any()):
                raise ValueError(f'face_crop: a box with a side outside [1, 2^24]: {b.tolist()}')
        return FaceCropFunction.apply(img, b.to(img.device, non_blocking=True).contiguous(), int(r))
    return face_crop_composite(img, box, r)


# ----------------------------------------------------------------------------- detector input
def detector_input_composite(img):
    mean = torch.tensor(DETECTOR_MEAN, device=img.device, dtype=img.dtype).view(1, 3, 1, 1)
    return ((img + 1) * 255 / 2).flip(-3) - mean


def detector_input_serves(img):
    return torch.is_tensor(img) and img.ndim == 4 and img.shape[1] == 3 and img.numel() > 0 and _f32_cuda(img)


def detector_input(img, fuse=None):
    """The face detector's input of img [N, 3, H, W] in [-1, 1]; never part of a graph (the detector runs under no_grad:
    its outputs only ever leave as host data)."""
    with torch.no_grad():
        if _fuse(fuse) and detector_input_serves(img):
            return _native.detector_input(img)
        return detector_input_composite(img)


# ----------------------------------------------------------------------------- heat-map distance
class HeatmapDistanceFunction(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, a, b):
        partial = _native.heatmap_distance_fwd(a, b)
        if partial is None:
            raise RuntimeError(f'heatmap_distance: no kernel for {tuple(a.shape)} (ask heatmap_distance_serves first)')
        ctx.save_for_backward(a, b)
        return partial.sum(1, dtype=torch.float64).to(torch.float32)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, grad):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad
        if not (need_a or need_b):
            return None, None
        out = _native.heatmap_distance_bwd(a, b, grad, need_a, need_b)
        if out is None:
            raise RuntimeError(f'heatmap_distance: no backward kernel for {tuple(a.shape)}')
        return out


def heatmap_distance_composite(a, b):
    return torch.sum(torch.square(a - b), dim=tuple(range(1, a.ndim)))


def heatmap_distance_serves(a, b):
    if not (torch.is_tensor(a) and torch.is_tensor(b) and a.ndim >= 2 and tuple(a.shape) == tuple(b.shape)):
        return False
    if not _f32_cuda(a, b) or a.shape[0] == 0:
        return False
    return _native.heatmap_distance_serves(a.shape[0], a.numel() // a.shape[0])


def heatmap_distance(a, b, fuse=None):
    """[N] = sum over everything but the batch axis of (a - b)^2 (Heat_Map_Loss before its mean; the heat-map score)."""
    if _fuse(fuse) and heatmap_distance_serves(a, b):
        return HeatmapDistanceFunction.apply(a, b)
    return heatmap_distance_composite(a, b)


# ----------------------------------------------------------------------------- landmark decode
def _center_scale(center, scale, batch, device):
    """(center [B, 2], scale [B]) float32 on `device` from tensors or the reference's lists (tensors and floats)."""
    if center is None or scale is None:
        return None, None
    if not torch.is_tensor(center):
        center = torch.stack([torch.as_tensor(c, dtype=torch.float32).reshape(2) for c in center])
    if not torch.is_tensor(scale):
        scale = torch.tensor([float(s) for s in scale], dtype=torch.float32)
    center = center.to(device=device, dtype=torch.float32, non_blocking=True).reshape(batch, 2).contiguous()
    scale = scale.to(device=device, dtype=torch.float32, non_blocking=True).reshape(batch).contiguous()
    return center, scale


def inverse_transform(points, center, scale, resolution):
    """transform(..., invert=True) of points [B, C, 2] in closed form, float32: (p - r * (-c / h + 0.5)) * h / r with
    h = 200 * scale, truncated toward zero and kept as float."""
    h = (200.0 * scale).reshape(-1, 1, 1)
    r = float(resolution)
    t = r * (-center.reshape(-1, 1, 2) / h + 0.5)
    return torch.trunc((points.to(torch.float32) - t) * h / r)


def landmark_decode_composite(hm, center=None, scale=None):
    """The decode from aten ops on whole tensors, any device, dtype and map size (at 64 x 64 the reference's: its interior
    test is written for that size): argmax with the first index on a tie, the quarter-pixel step toward the larger
    neighbour, minus a half."""
    b, c, h, w = hm.shape
    flat = hm.reshape(b, c, h * w)
    idx = torch.argmax(flat, dim=-1)
    px, py = idx % w, idx // w
    inside = (px > 0) & (px < w - 1) & (py > 0) & (py < h - 1)
    last = h * w - 1

    def at(offset):
        return flat.gather(-1, (idx + offset).clamp(0, last).unsqueeze(-1)).squeeze(-1)
    dx = torch.where(inside, torch.sign(at(1) - at(-1)) * 0.25, 0.0)
    dy = torch.where(inside, torch.sign(at(w) - at(-w)) * 0.25, 0.0)
    dtype = hm.dtype if hm.is_floating_point() else torch.float32
    preds = torch.stack((px.to(dtype) + 1 + dx.to(dtype), py.to(dtype) + 1 + dy.to(dtype)), dim=-1) - 0.5
    center, scale = _center_scale(center, scale, b, hm.device)
    if center is None:
        return preds, torch.zeros_like(preds)
    return preds, inverse_transform(preds, center, scale, h).to(dtype)


def landmark_decode_serves(hm):
    return torch.is_tensor(hm) and hm.ndim == 4 and tuple(hm.shape[2:]) == (HEATMAP_SIZE, HEATMAP_SIZE) \
        and hm.shape[0] * hm.shape[1] > 0 and _f32_cuda(hm)


def landmark_decode(hm, center=None, scale=None, fuse=None):
    """(preds, preds_orig), each [B, C, 2]: the maxima of the heat maps hm [B, C, H, W] in map coordinates and, with
    center ([B, 2] or a list of B points) and scale ([B] or a list of B numbers), in the image's frame (zeros without)."""
    with torch.no_grad():
        if _fuse(fuse) and landmark_decode_serves(hm):
            center, scale = _center_scale(center, scale, hm.shape[0], hm.device)
            out = _native.landmark_decode(hm, center, scale)
            if out is None:
                raise RuntimeError(f'landmark_decode: no kernel for maps {tuple(hm.shape)}')
            return out
        return landmark_decode_composite(hm, center, scale)
