"""LPIPS distance of one VGG tap on the MI355X kernel (lpips/__init__.py, PNetLin.forward).

    u_k  = f_k / (sqrt(sum_c f_k^2) + eps)                    (per pixel, k = 0, 1)
    d[n] = mean over pixels of sum_c w_c (u0_c - u1_c)^2      (the 1x1 conv to one channel, then the spatial mean)

One kernel pass per direction (csrc/lpips_distance.hip): the forward reads both features once and leaves fixed-order
per-block partial sums; the backward reads both again, recomputes the norms and writes the wanted gradients once.  The
composite it replaces is about ten aten passes per direction over feature-sized tensors and keeps several of them for
autograd; this Function saves the two features (which the VGG trunk's own backward holds anyway) and nothing else.
Nothing synchronises with the host.  The 1x1 weight is frozen: it gets no gradient.  The term is first order only (it is
never on an R1 or path-length graph), hence once_differentiable.

The kernel serves float32, NHWC-dense features of 64 / 128 / 256 / 512 channels; `lpips_distance` evaluates the composite
for everything else (bf16 features under autocast, NCHW features, CPU tensors, a weight that wants a gradient).
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from ._native import amp_fwd as _amp_fwd, amp_bwd as _amp_bwd


class LpipsDistanceFunction(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, f0, f1, weight, eps):
        d = _native.lpips_distance(f0, f1, weight, eps)
        if d is None:
            raise RuntimeError(f'lpips_distance: no kernel for features {tuple(f0.shape)} at {f0.data_ptr():#x} / '
                               f'{f1.data_ptr():#x} (ask lpips_distance_serves first)')
        ctx.save_for_backward(f0, f1, weight)
        ctx.eps = eps
        return d.view(-1, 1, 1, 1)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, grad_d):
        f0, f1, weight = ctx.saved_tensors
        need0, need1 = ctx.needs_input_grad[:2]
        if not (need0 or need1):
            return None, None, None, None
        grads = _native.lpips_distance_backward(f0, f1, weight, grad_d, need0, need1, ctx.eps)
        if grads is None:
            raise RuntimeError(f'lpips_distance: no backward kernel for features {tuple(f0.shape)}')
        return grads[0], grads[1], None, None


def lpips_distance_composite(f0, f1, weight, eps=1e-10):
    """The aten form, operation for operation that of PNetLin.forward: [N, 1, 1, 1]."""
    u0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + eps)
    u1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + eps)
    return F.conv2d((u0 - u1) ** 2, weight).mean([2, 3], keepdim=True)


def lpips_distance_serves(f0, f1, weight):
    """Does the kernel take this call?  CUDA float32 features of one shape, NHWC-dense and 16-byte aligned, a channel
    count the kernel is built for, autocast off, and a frozen [1, C, 1, 1] weight."""
    if not (torch.is_tensor(f0) and torch.is_tensor(f1) and f0.is_cuda and f1.is_cuda and weight.is_cuda):
        return False
    if torch.is_autocast_enabled():
        return False
    if f0.dtype != torch.float32 or f1.dtype != torch.float32 or weight.dtype != torch.float32:
        return False
    if f0.ndim != 4 or f0.shape != f1.shape or f0.device != f1.device or weight.device != f0.device:
        return False
    if tuple(weight.shape) != (1, f0.shape[1], 1, 1) or weight.requires_grad:
        return False
    if not (_native.nhwc_dense(f0) and _native.nhwc_dense(f1)):
        return False
    if (f0.data_ptr() | f1.data_ptr() | weight.data_ptr()) % 16:
        return False
    n, c, h, w = f0.shape
    return n > 0 and 0 < h * w < 2 ** 31 and _native.lib().fmgan_lpips_distance_blocks(n, c, h * w) > 0


def lpips_distance(f0, f1, weight, eps=1e-10):
    """[N, 1, 1, 1] LPIPS distance of one tap: f0, f1 [N, C, H, W] features, weight [1, C, 1, 1] the 1x1 conv's;
    differentiable w.r.t. both features.  The kernel where lpips_distance_serves(), the aten composite elsewhere."""
    if lpips_distance_serves(f0, f1, weight):
        return LpipsDistanceFunction.apply(f0, f1, weight, eps)
    return lpips_distance_composite(f0, f1, weight, eps)
