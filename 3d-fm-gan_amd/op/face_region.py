"""Face-regional loss of the dual-supervision G step on the MI355X kernel (reference Util/training_util.py:228-256).

    mask  = mean_c(render) > -1                      (where the render shows a face; its background is -1)
    loss  = mean((render*mask - image*mask)^2)       over [N, C, H, W], the reference's torch.mean
    score = the same mean per sample                 (Evaluation/quant_eval.py:167-172, face_diff_score)

One kernel pass per direction (csrc/face_region.hip): the forward reads render and image once and leaves fixed-order
per-block partial sums; the backward reads the upstream gradient from device memory.  Nothing synchronises with the
host, and the mask never leaves the GPU (the reference copies it to the CPU and back in every call).  Renders are data:
they get no gradient.  The term is first order only (it is never on an R1 or path-length graph), hence
once_differentiable.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from ._native import amp_fwd as _amp_fwd, amp_bwd as _amp_bwd


class FaceRegionLossFunction(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, render, image):
        s = _native.face_region_loss(render, image)
        ctx.save_for_backward(render, image)
        return s.sum() / image.numel()

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, grad_loss):
        render, image = ctx.saved_tensors
        grad_image = _native.face_region_loss_backward(render, image, grad_loss) if ctx.needs_input_grad[1] else None
        return None, grad_image


def face_region_loss(render, image):
    """0-dim mean((render*m - image*m)^2), m = mean_c(render) > -1; differentiable w.r.t. `image`."""
    return FaceRegionLossFunction.apply(render, image)


def face_region_scores(render, image):
    """Per-sample face difference [N] = mean over (C, H, W) of (render*m - image*m)^2 (quant_eval.py's face_diff_score);
    evaluation only, no autograd."""
    with torch.no_grad():
        return _native.face_region_loss(render, image) / image[0].numel()
