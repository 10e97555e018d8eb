"""Input stage of the perceptual path length (reference Evaluation/ppl.py:116-123 and the script's :191-202): from the
Generator's interleaved image batch [2P, 3, S, S] (sample 2p / 2p+1: the two images of pair p) to the two inputs of the
LPIPS trunk.

    crop (optional)   c = S // 8, rows 3c:7c, columns 2c:6c                         -> S' = 4c
    resample          factor = S' // 256; bilinear (align_corners=False) to 256^2 only when factor > 1
    split             image[::2], image[1::2]
    scale             lpips.ScalingLayer: (x - shift) / scale
    layout            channels_last, the layout the trunk converts to on entry

pair_input(image, scaling_layer) gives (in0, in1) for PerceptualLoss.forward_scaled.  On the MI355X kernel
(csrc/ppl_input.hip) that is one launch which reads only the source pixels it needs and writes the two trunk inputs;
pair_input_composite is the same from slicing, F.interpolate and the module (five to eight launches), for what the
kernel does not serve: CPU tensors, other dtypes or layouts, non-square images, sizes whose reduction is not by 2 or 4
(S' = 768).  At factor 2 and 4 both interpolation weights are 1/2; the kernel's association of the four products is fixed
(include/fmgan_hip.h) and may differ from aten's in the last bit.  Inference only: there is no autograd.
"""
import torch
import torch.nn.functional as F

from . import _native

TARGET = _native.LPIPS_SIZE


def _refuse_grad(image):
    if torch.is_grad_enabled() and image.requires_grad:
        raise RuntimeError('pair_input: inference only (no autograd): call under torch.no_grad() or detach the images; '
                           'the training path uses Util.training_util.LPIPS_Loss')


def pair_geometry(height, width, crop=False):
    """((y0, x0, hc, wc), factor): the window the reference keeps of an image and the factor it reduces it by."""
    if crop:
        c = height // 8
        y0, x0 = 3 * c, 2 * c
        hc, wc = min(7 * c, height) - y0, max(min(6 * c, width) - x0, 0)
    else:
        y0, x0, hc, wc = 0, 0, height, width
    return (y0, x0, hc, wc), hc // TARGET


def pair_input_plan(shape, crop):
    """(window, f) with which the kernel gives the composite's tensors, or None: square images only, reduction to 256^2 by
    exactly 2 or 4, or no reduction at all."""
    if len(shape) != 4 or shape[1] != 3 or shape[0] == 0 or shape[0] % 2 != 0 or shape[2] != shape[3]:
        return None
    window, factor = pair_geometry(shape[2], shape[3], crop)
    if window[2] <= 0 or window[2] != window[3]:
        return None
    if factor <= 1:
        return window, 1
    if factor in (2, 4) and window[2] == TARGET * factor:
        return window, factor
    return None


def pair_input_serves(image, crop=False):
    """Does the kernel take this batch (host logic, nothing runs)?  A [2P, 3, S, S] float32 contiguous GPU tensor whose
    (cropped) size S' is 256 * factor with factor 2 or 4, or any size with factor <= 1 (no resampling), and whose launch
    the library plans (fmgan_lpips_pair_input_select > 0)."""
    if not (torch.is_tensor(image) and image.is_cuda and image.dtype == torch.float32 and image.is_contiguous()):
        return False
    plan = pair_input_plan(tuple(image.shape), crop)
    if plan is None:
        return False
    (y0, x0, hc, wc), f = plan
    return _native.lib().fmgan_lpips_pair_input_select(image.shape[0] // 2, image.shape[2], image.shape[3], y0, x0, hc, wc,
                                                       f) > 0


def pair_resize(image, crop=False):
    """The reference's crop and reduction of the whole interleaved batch (any device and dtype)."""
    (y0, x0, hc, wc), factor = pair_geometry(image.shape[2], image.shape[3], crop)
    if crop:
        image = image[:, :, y0:y0 + hc, x0:x0 + wc]
    if factor > 1:
        image = F.interpolate(image, size=(TARGET, TARGET), mode='bilinear', align_corners=False)
    return image


def pair_input_composite(image, scaling_layer, crop=False):
    """(in0, in1) from slicing, F.interpolate and the module, on any device and dtype; scaling_layer None: no scaling."""
    _refuse_grad(image)
    with torch.no_grad():
        image = pair_resize(image, crop)
        halves = []
        for half in (image[::2], image[1::2]):
            if scaling_layer is not None:
                half = scaling_layer(half)
            halves.append(half.contiguous(memory_format=torch.channels_last))
    return tuple(halves)


def pair_input(image, scaling_layer, crop=False, fuse=True):
    """(in0, in1): the kernel where it serves the batch (and `fuse`), the composite elsewhere."""
    _refuse_grad(image)
    if fuse and scaling_layer is not None and pair_input_serves(image, crop):
        shift, scale = scaling_layer.shift, scaling_layer.scale
        if all(t.is_cuda and t.dtype == torch.float32 and t.device == image.device for t in (shift, scale)):
            window, f = pair_input_plan(tuple(image.shape), crop)
            with torch.no_grad():
                out = _native.lpips_pair_input(image, shift, scale, window, f)
            if out is not None:
                return out
    return pair_input_composite(image, scaling_layer, crop)
