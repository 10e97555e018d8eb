"""Metric stage of the quantitative evaluation (reference Evaluation/quant_eval.py:25-49, 100).

    gray_x = Convert_Tensor_For_Face_Recognition_Loss(x)          the ArcFace network's input, [N, 1, H/k, W/k]
    l1     = mean |a - b| over (C, H, W)                          per sample, [N]

face_input(a, b) gives the grey image of `a` and, as asked, that of `b` and the L1 between them.  On the MI355X kernel
(csrc/eval_scores.hip) that is one launch reading every element once; face_input_composite is the same from
Convert_Tensor_For_Face_Recognition_Loss and torch ops (~22 launches for a pair), for tensors the kernel does not serve:
CPU tensors, other dtypes or layouts, pooling factors other than 1 / 2 / 4 / 8.  The grey images of the two forms are equal
bit for bit (the kernel adds in the composite's order); the L1 sums differ in their summation order only.
Inference only: there is no autograd.
"""
import torch

from . import _native


def _refuse_grad(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError('face_input: inference only (no autograd): call under torch.no_grad() or detach the images; '
                           'the training path uses Util.training_util.Face_Identity_Loss / L1_Loss')


def face_input_serves(a, b=None):
    """Does the kernel take these tensors (host logic, nothing runs)?  [N, 3, H, W] float32 contiguous GPU tensors of one
    shape whose pooling factor and size the library serves (fmgan_face_input_blocks > 0)."""
    for t in (a, b):
        if t is None:
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.ndim == 4 and t.shape[1] == 3
                and t.is_contiguous() and tuple(t.shape) == tuple(a.shape)):
            return False
    n, _, h, w = a.shape
    return n > 0 and _native.lib().fmgan_face_input_blocks(n, h, w, _native.face_input_pool(w)) > 0


def face_input_composite(a, b=None, want_gray_b=False, want_l1=False):
    """(gray_a, gray_b or None, l1 or None) from Convert_Tensor_For_Face_Recognition_Loss and torch ops, on any device."""
    from Util.training_util import Convert_Tensor_For_Face_Recognition_Loss
    if b is None and (want_gray_b or want_l1):
        raise ValueError('face_input: gray_b / l1 asked for without a second image')
    _refuse_grad(a, b)
    with torch.no_grad():
        gray_a = Convert_Tensor_For_Face_Recognition_Loss(a)
        gray_b = Convert_Tensor_For_Face_Recognition_Loss(b) if want_gray_b else None
        l1 = torch.mean(torch.abs(a - b), dim=(1, 2, 3)) if want_l1 else None
    return gray_a, gray_b, l1


def face_input(a, b=None, want_gray_b=False, want_l1=False, fuse=True):
    """(gray_a, gray_b or None, l1 or None): the kernel where it serves the tensors (and `fuse`), the composite
    elsewhere."""
    _refuse_grad(a, b)
    if fuse and face_input_serves(a, b):
        with torch.no_grad():
            out = _native.face_input(a, b, want_gray_b, want_l1)
        if out is not None:
            return out
    return face_input_composite(a, b, want_gray_b, want_l1)
