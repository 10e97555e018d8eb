"""Input stage of the FID's Inception network (reference Evaluation/inception.py:155-162): from the Generator's image
batch [B, 3, S, S] to the network's input.

    resample     F.interpolate(size=(299, 299), mode='bilinear', align_corners=False)      (resize_input)
    normalize    2x - 1                                                                     (normalize_input)
    layout       channels_last, the layout the folded forward runs in

On the MI355X kernel (csrc/inception_input.hip) that is one launch which reads only tap pixels and writes the input once;
inception_input_composite is the same from F.interpolate and torch arithmetic, for what the kernel does not serve: CPU
tensors, other dtypes or layouts, sizes other than 256 / 512 / 1024 / 299, non-square images, resize_input=False at
another size than 299.  The kernel follows aten's fp32 index and weight rule (include/fmgan_hip.h); the association of the
four products is fixed there and may differ from aten's kernel in the last bits.  Inference only: there is no autograd.
"""
import torch
import torch.nn.functional as F

from . import _native

SIZE = _native.INCEPTION_SIZE
SERVED_SIZES = (256, 512, 1024, SIZE)


def _refuse_grad(image):
    if torch.is_grad_enabled() and image.requires_grad:
        raise RuntimeError('inception_input: inference only (no autograd): call under torch.no_grad() or detach the '
                           'images')


def inception_input_serves(image, resize_input=True):
    """Does the kernel take this batch (host logic, nothing runs)?  A [B, 3, S, S] float32 contiguous GPU tensor with S
    in SERVED_SIZES (S = 299 alone without resize_input) whose launch the library plans."""
    if not (torch.is_tensor(image) and image.is_cuda and image.dtype == torch.float32 and image.is_contiguous()):
        return False
    if image.ndim != 4 or image.shape[1] != 3 or image.shape[0] == 0 or image.shape[2] != image.shape[3]:
        return False
    if image.shape[2] not in SERVED_SIZES or (not resize_input and image.shape[2] != SIZE):
        return False
    return _native.lib().fmgan_inception_input_select(image.shape[0], image.shape[2], image.shape[3]) > 0


def inception_input_composite(image, normalize_input=True, resize_input=True):
    """The stage from F.interpolate and torch arithmetic, on any device and dtype, as the reference writes it."""
    _refuse_grad(image)
    with torch.no_grad():
        if resize_input:
            image = F.interpolate(image, size=(SIZE, SIZE), mode='bilinear', align_corners=False)
        if normalize_input:
            image = 2 * image - 1
        return image.contiguous(memory_format=torch.channels_last)


def inception_input(image, normalize_input=True, resize_input=True, fuse=True):
    """The network's input in channels_last storage: the kernel where it serves the batch (and `fuse`), the composite
    elsewhere."""
    _refuse_grad(image)
    if fuse and inception_input_serves(image, resize_input):
        with torch.no_grad():
            out = _native.inception_input(image, normalize_input)
        if out is not None:
            return out
    return inception_input_composite(image, normalize_input, resize_input)
