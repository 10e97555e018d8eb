"""Image stage of the projection criterion (reference Evaluation/image_projection/project/__init__.py:125-129, 199-220):
what stands between the Generator's image and the loss value on one side and the LPIPS trunk on the other.

    sq_sum    = sum((x - target)^2)                 or  sum((x - target)^2 * mask)   (weighted_mse_loss's numerator)
    y_scaled  = ScalingLayer(F.interpolate(clamp(x, -1, 1), size=256, mode='bilinear', align_corners=False))

projection_stage(x, target, mask, scaling_layer, want_y) gives (sq_sum, y_scaled or None) under autograd with respect to
x.  On the MI355X kernels (csrc/projection_loss.hip) that is one launch forward, which reads x and target once and
writes fixed-order partial sums (added here in float64: sq_sum is bit-reproducible) and the trunk input in channels_last
storage, and one launch backward, which reads x, target and the trunk's gradient and writes grad_x; only x and target are
kept for the backward.  The composite is about eight launches per direction and keeps their intermediates.  Nothing
synchronises with the host: the upstream gradient of sq_sum goes to the kernel as a device scalar.

projection_stage_composite is the same mathematics from aten ops on any device, dtype and size, including the reference's
upsampling to 256 for smaller images; projection_stage_serves says whether the kernels take a call: float32 contiguous
CUDA tensors, [B, 3, S, S] with S in {256, 512, 1024}, autocast off, target and mask without a gradient.  At S = 512 and
1024 both interpolation weights are 1/2; the kernel's association of the four products is fixed (include/fmgan_hip.h)
and may differ from aten's in the last bit.  As in the reference the mask multiplies: a NaN under a zero of the mask still
reaches the sum and its own gradient element.  First order only (the projection loop never differentiates twice), hence
once_differentiable: a double backward raises.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from ._native import amp_fwd as _amp_fwd, amp_bwd as _amp_bwd

TARGET = _native.LPIPS_SIZE
SIZES = (256, 512, 1024)


class ProjectionStageFunction(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, target, mask, shift, scale, want_y):
        out = _native.projection_loss_fwd(x, target, mask, shift, scale, want_y)
        if out is None:
            raise RuntimeError(f'projection_stage: no kernel for images {tuple(x.shape)} (ask projection_stage_serves '
                               f'first)')
        partial, y = out
        ctx.save_for_backward(x, target, mask, scale)
        ctx.set_materialize_grads(False)
        sq_sum = partial.sum(dtype=torch.float64).to(torch.float32)
        if y is None:
            return sq_sum, None
        return sq_sum, y

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, grad_sq, grad_y):
        x, target, mask, scale = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (grad_sq is None and grad_y is None):
            return None, None, None, None, None, None
        if grad_sq is None:
            k = torch.zeros((1,), dtype=torch.float32, device=x.device)
        else:
            k = (grad_sq.to(device=x.device, dtype=torch.float32) * 2).reshape(1)
        if grad_y is not None:
            grad_y = grad_y.to(torch.float32).contiguous(memory_format=torch.channels_last)
        grad_x = _native.projection_loss_bwd(x, target, mask, grad_y, k, scale)
        if grad_x is None:
            raise RuntimeError(f'projection_stage: no backward kernel for images {tuple(x.shape)}')
        return grad_x, None, None, None, None, None


def projection_resize(image, size=TARGET):
    """clamp to [-1, 1], then the reference's bilinear resampling to size x size (up or down; any device and dtype)."""
    return F.interpolate(torch.clamp(image, -1., 1.), size=size, mode='bilinear', align_corners=False)


def projection_trunk_input(image, scaling_layer, size=TARGET):
    """The LPIPS trunk's input of an image from aten ops: clamp, resample to size x size, ScalingLayer (None: left out)."""
    y = projection_resize(image, size)
    return y if scaling_layer is None else scaling_layer(y)


def projection_stage_composite(x, target, mask, scaling_layer, want_y=True, size=TARGET):
    """(sq_sum, y_scaled or None) from aten ops, operation for operation the reference's: differentiable to any order."""
    sq = (x - target) ** 2
    if mask is not None:
        sq = sq * mask.expand_as(sq)
    return sq.sum(), (projection_trunk_input(x, scaling_layer, size) if want_y else None)


def projection_stage_serves(x, target, mask=None, scaling_layer=None):
    """Do the kernels take this call (host logic, nothing runs)?"""
    if not (torch.is_tensor(x) and torch.is_tensor(target) and x.is_cuda and x.ndim == 4):
        return False
    if torch.is_autocast_enabled() or target.requires_grad or (mask is not None and mask.requires_grad):
        return False
    tensors = [x, target] + ([mask] if mask is not None else [])
    if scaling_layer is not None:
        tensors += [scaling_layer.shift, scaling_layer.scale]
        if scaling_layer.shift.numel() != 3 or scaling_layer.scale.numel() != 3:
            return False
    if any(t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() for t in tensors):
        return False
    b, c, h, w = x.shape
    if c != 3 or h != w or h not in SIZES or tuple(target.shape) != tuple(x.shape):
        return False
    if mask is not None and tuple(mask.shape) != (h, w):
        return False
    return b > 0 and _native.lib().fmgan_projection_loss_select(b, h, w, h // TARGET) > 0


def projection_stage(x, target, mask, scaling_layer, want_y=True, fuse=True, size=TARGET):
    """(sq_sum, y_scaled or None): the kernels where projection_stage_serves() (and `fuse`, and size 256), the composite
    elsewhere.  want_y needs the scaling_layer (lpips.ScalingLayer) on the fused path; sq_sum is a 0-dim tensor of x's
    dtype."""
    if fuse and size == TARGET and (scaling_layer is not None or not want_y) \
            and projection_stage_serves(x, target, mask, scaling_layer):
        if scaling_layer is None:
            shift = scale = torch.ones((3,), dtype=torch.float32, device=x.device)
        else:
            shift, scale = scaling_layer.shift.reshape(3), scaling_layer.scale.reshape(3)
        return ProjectionStageFunction.apply(x, target, mask, shift, scale, bool(want_y))
    return projection_stage_composite(x, target, mask, scaling_layer, want_y, size)
