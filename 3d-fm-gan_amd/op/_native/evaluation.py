"""The evaluation stages: csrc/eval_scores.hip, fid_stats.hip, inception_input.hip."""
import torch

from .core import (
    check, FMGAN_EUNSUPPORTED, fp, launching, lib, _nhwc_empty, require_f32_gpu, require_gpu, served)


# ----------------------------------------------------------------------------- csrc/eval_scores.hip
def face_input_pool(width, face_size=128):
    """Pooling factor of Convert_Tensor_For_Face_Recognition_Loss for images `width` wide."""
    return max(1, width // face_size)


def face_input(a, b=None, want_gray_b=False, want_l1=False, face_size=128):
    """Metric stage of the quantitative evaluation in one launch (csrc/eval_scores.hip): a, b [B, 3, H, W] f32 contiguous
    -> (gray_a, gray_b or None, l1 or None): gray_x [B, 1, H/k, W/k] is Convert_Tensor_For_Face_Recognition_Loss(x) with
    k = face_input_pool(W), l1 [B] = mean |a - b| over (C, H, W) from fixed-order partials (bit-reproducible).  None
    (alone) when the kernel does not serve the shape (k not 1 / 2 / 4 / 8, H or W no multiple of k): the caller then
    evaluates the composite.  Tensors of another dtype, device or layout are refused (RuntimeError), as is C != 3 or a `b`
    of another shape (ValueError)."""
    if a.ndim != 4 or a.shape[1] != 3 or (b is not None and tuple(b.shape) != tuple(a.shape)):
        got = f'a {tuple(a.shape)}' + ('' if b is None else f' and b {tuple(b.shape)}')
        raise ValueError(f'face_input: {got}: expected [N, 3, H, W] tensors of one shape')
    if b is None and (want_gray_b or want_l1):
        raise ValueError('face_input: gray_b / l1 asked for without a second image')
    require_f32_gpu('face_input', ((a, 'a'), (b, 'b')))
    n, _, h, w = a.shape
    k = face_input_pool(w, face_size)
    if n == 0:
        return None
    blocks = lib().fmgan_face_input_blocks(n, h, w, k)
    if blocks <= 0:
        return None
    if not (want_gray_b or want_l1):
        b = None
    gray_a = torch.empty((n, 1, h // k, w // k), dtype=torch.float32, device=a.device)
    gray_b = torch.empty_like(gray_a) if want_gray_b else None
    partial = torch.empty((n, blocks), dtype=torch.float32, device=a.device) if want_l1 else None
    with launching(a, 'face_input', (n, h, w, k, b is not None)) as stream:
        st = lib().fmgan_face_input_f32(fp(a), fp(b), fp(gray_a), fp(gray_b), fp(partial), n, h, w, k, stream)
    if not served(st, 'face_input'):
        return None
    return gray_a, gray_b, (partial.sum(1) / (3 * h * w) if want_l1 else None)


# ----------------------------------------------------------------------------- csrc/fid_stats.hip
def f64p(t, name, device):
    """data_ptr of a contiguous float64 GPU tensor on `device` (the f64 state of op/fid_stats.py travels by pointer)."""
    if t.dtype != torch.float64 or not t.is_cuda or t.device != device or not t.is_contiguous():
        raise RuntimeError(f'{name}: expected a contiguous float64 tensor on {device}, got {t.dtype} on {t.device} with '
                           f'strides {t.stride()}')
    return t.data_ptr()


def fid_stats_serves(b, d):
    """Does the update kernel take a [b, d] batch (host logic, nothing runs)?"""
    return lib().fmgan_fid_stats_select(int(b), int(d)) > 0


def fid_stats_update(feat, shift, total, outer):
    """One batch into the running moments, in place, one launch (csrc/fid_stats.hip): feat [b, d] f32 contiguous, shift /
    total [d] and outer [d, d] f64 on feat's device; y = feat - shift in f64, total += sum_b y, outer[i][j] += sum_b y_i y_j
    for i <= j.  False (nothing written) when the library declines the shape (d % 16 != 0): the caller then evaluates the
    composite."""
    if feat.ndim != 2 or tuple(shift.shape) != (feat.shape[1],) or tuple(total.shape) != tuple(shift.shape) or \
            tuple(outer.shape) != (feat.shape[1],) * 2:
        raise ValueError(f'fid_stats_update: feat {tuple(feat.shape)}, shift {tuple(shift.shape)}, sum '
                         f'{tuple(total.shape)}, outer {tuple(outer.shape)}: expected [b, d], [d], [d], [d, d]')
    require_f32_gpu('fid_stats_update', ((feat, 'feat'),))
    b, d = feat.shape
    ps, pt, po = (f64p(t, f'fid_stats_update: {n}', feat.device) for t, n in ((shift, 'shift'), (total, 'sum'),
                                                                                (outer, 'outer')))
    if b == 0 or not fid_stats_serves(b, d):
        return False
    with launching(feat, 'fid_stats', (b, d, 0)) as stream:
        st = lib().fmgan_fid_stats_update_f32(fp(feat), ps, pt, po, b, d, stream)
    return served(st, 'fid_stats_update')


def fid_stats_finish(total, outer, shift, n):
    """(mean [d], cov [d, d]) f64 from the running moments of n samples, one launch; cov is exactly symmetric."""
    d = total.shape[0]
    if tuple(shift.shape) != (d,) or tuple(outer.shape) != (d, d):
        raise ValueError(f'fid_stats_finish: sum {tuple(total.shape)}, shift {tuple(shift.shape)}, outer '
                         f'{tuple(outer.shape)}: expected [d], [d], [d, d]')
    require_gpu(total, 'sum')
    pt, po, ps = (f64p(t, f'fid_stats_finish: {nm}', total.device) for t, nm in ((total, 'sum'), (outer, 'outer'),
                                                                                 (shift, 'shift')))
    mean = torch.empty((d,), dtype=torch.float64, device=total.device)
    cov = torch.empty((d, d), dtype=torch.float64, device=total.device)
    with launching(total, 'fid_stats', (int(n), d, 1)) as stream:
        st = lib().fmgan_fid_stats_finish_f64(pt, po, ps, int(n), mean.data_ptr(), cov.data_ptr(), d, stream)
    check(st, 'fid_stats_finish')
    return mean, cov


# ----------------------------------------------------------------------------- csrc/inception_input.hip
INCEPTION_SIZE = 299                      # the size the FID's Inception network is evaluated at


def inception_input(image, normalize):
    """Input stage of the FID's Inception network in one launch (csrc/inception_input.hip): image [B, 3, S, S] f32
    contiguous -> [B, 3, 299, 299] in channels_last storage: F.interpolate(bilinear, align_corners=False) by aten's fp32
    rule, then 2x - 1 when `normalize`.  None when the library declines (S outside 256 / 512 / 1024 / 299, not square):
    the caller then evaluates the composite.  Tensors of another dtype, device or layout are refused (RuntimeError), as
    is another shape (ValueError)."""
    if image.ndim != 4 or image.shape[1] != 3:
        raise ValueError(f'inception_input: image {tuple(image.shape)}: expected [B, 3, S, S]')
    require_f32_gpu('inception_input', ((image, 'image'),))
    b, _, h, w = image.shape
    if b == 0 or lib().fmgan_inception_input_select(b, h, w) == FMGAN_EUNSUPPORTED:
        return None
    with launching(image, 'inception_input', (b, h, w, bool(normalize))) as stream:
        out = _nhwc_empty(b, 3, INCEPTION_SIZE, INCEPTION_SIZE, image.device)
        st = lib().fmgan_inception_input_f32(fp(image), fp(out), b, h, w, int(bool(normalize)), stream)
    return out if served(st, 'inception_input') else None
