"""The loss stages: csrc/face_region.hip, lpips_distance.hip, ppl_input.hip, projection_loss.hip, landmark.hip."""
import torch

from .core import (
    check, FMGAN_EUNSUPPORTED, fp, launching, lib, nhwc_dense, _nhwc_empty, require_f32_gpu, served)


LPIPS_SIZE = 256                          # the size LPIPS is evaluated at (TARGET of op.ppl_input, op.projection_loss)


# ----------------------------------------------------------------------------- csrc/face_region.hip
def _face_region_shape(r, g):
    """(r, g) contiguous, (B, C, H*W) — after the checks shared by the three face-region entry points: shapes first
    (ValueError naming both, before anything touches a device), then device and dtype (RuntimeError, no fallback)."""
    if r.ndim != 4 or (g is not None and tuple(r.shape) != tuple(g.shape)):
        got = f'render {tuple(r.shape)}' + ('' if g is None else f' and image {tuple(g.shape)}')
        raise ValueError(f'face_region: {got}: expected [N, C, H, W] tensors of one shape (the face-regional loss '
                         f'compares the render with the generated image pixel by pixel; renders are not resampled)')
    require_f32_gpu('face_region', ((r, 'render'), (g, 'image')), contiguous=False, same_device=False)
    r = r.contiguous()
    g = g.contiguous() if g is not None else None
    b, c, h, w = r.shape
    return r, g, (b, c, h * w)


def face_region_loss(r, g):
    """Per-sample sums S[b] = sum_{c,y,x} m * (r - g)^2 with m = mean_c(r) > -1 (Util/training_util.py:228-256):
    r (render), g (generated image) [B, C, H, W] f32 of one shape -> S [B] f32.  Fixed-order per-block partials from
    the kernel, summed here: bit-reproducible.  loss = S.sum() / numel; face_diff_score = S / (C*H*W)."""
    r, g, (b, c, hw) = _face_region_shape(r, g)
    partial = torch.empty((b, lib().fmgan_face_region_blocks(b, hw)), dtype=torch.float32, device=r.device)
    with launching(r, 'face_region', (b, c, hw, 0)) as stream:
        st = lib().fmgan_face_region_loss_f32(fp(r), fp(g), fp(partial), b, c, hw, stream)
    check(st, 'face_region_loss')
    return partial.sum(1)


def face_region_loss_backward(r, g, grad_loss):
    """Gradient of mean(m * (r - g)^2) w.r.t. g: grad_loss * 2/numel * m * (g - r), exactly 0 outside the mask.
    grad_loss: the upstream gradient as a one-element f32 tensor ON THE DEVICE, read by the kernel (no .item())."""
    r, g, (b, c, hw) = _face_region_shape(r, g)
    gl = grad_loss.reshape(-1)
    if gl.numel() != 1:
        raise ValueError(f'face_region_loss_backward: grad_loss must hold one element, got {tuple(grad_loss.shape)}')
    gl = gl.to(device=r.device, dtype=torch.float32).contiguous()
    dg = torch.empty_like(g)
    with launching(r, 'face_region', (b, c, hw, 1)) as stream:
        st = lib().fmgan_face_region_backward_f32(fp(r), fp(g), fp(gl), fp(dg), b, c, hw, stream)
    check(st, 'face_region_loss_backward')
    return dg


def render_mask(r):
    """Get_Render_Mask (Util/training_util.py:228-238) on the GPU: r [N, C, H, W] f32 -> float 0/1 mask [N, H, W]
    (mean_c(r) > -1, the same decision as torch's r.mean(1) > -1 on the same device)."""
    r, _, (b, c, hw) = _face_region_shape(r, None)
    mask = torch.empty((b, r.shape[2], r.shape[3]), dtype=torch.float32, device=r.device)
    with launching(r, 'face_region', (b, c, hw, 2)) as stream:
        st = lib().fmgan_render_mask_f32(fp(r), fp(mask), b, c, hw, stream)
    check(st, 'render_mask')
    return mask


# ----------------------------------------------------------------------------- csrc/lpips_distance.hip
def _lpips_distance_shape(f0, f1, w):
    """(N, C, H*W) after the checks shared by the two LPIPS-distance entry points: shapes and layout first (ValueError),
    then device and dtype (RuntimeError from fp(), no fallback)."""
    if f0.ndim != 4 or tuple(f0.shape) != tuple(f1.shape) or w.numel() != f0.shape[1]:
        raise ValueError(f'lpips_distance: features {tuple(f0.shape)} and {tuple(f1.shape)}, weight {tuple(w.shape)}: '
                         f'expected two [N, C, H, W] tensors of one shape and C weights')
    if not (nhwc_dense(f0) and nhwc_dense(f1)):
        raise ValueError('lpips_distance: features must be NHWC-dense (channels_last storage); the kernel reads a '
                         'pixel\'s channel vector as one contiguous run')
    n, c, h, wd = f0.shape
    return n, c, h * wd


def lpips_distance(f0, f1, w, eps=1e-10):
    """LPIPS distance of one tap: f0, f1 [N, C, H, W] f32, NHWC-dense; w the C weights of the 1x1 conv (any shape)
    -> d [N] = mean_p sum_c w_c (u0 - u1)^2 with u = f / (sqrt(sum_c f^2) + eps).  Fixed-order per-block partials from
    the kernel, summed here: bit-reproducible.  None when the kernel does not serve the shape (C not 64 / 128 / 256 /
    512, pointers not 16-byte aligned): the caller then evaluates the composite."""
    n, c, hw = _lpips_distance_shape(f0, f1, w)
    w = w.contiguous()
    p0, p1, pw = fp(f0), fp(f1), fp(w)
    if n == 0:
        return torch.zeros((0,), dtype=torch.float32, device=f0.device)
    blocks = lib().fmgan_lpips_distance_blocks(n, c, hw)
    if blocks <= 0:
        return None
    partial = torch.empty((n, blocks), dtype=torch.float32, device=f0.device)
    with launching(f0, 'lpips_distance', (n, c, hw, 0)) as stream:
        st = lib().fmgan_lpips_distance_f32(p0, p1, pw, fp(partial), n, c, hw, float(eps), stream)
    return partial.sum(1) / hw if served(st, 'lpips_distance') else None


def lpips_distance_backward(f0, f1, w, grad, need0, need1, eps=1e-10):
    """Data gradients of lpips_distance: grad [N] is the upstream gradient of d ON THE DEVICE, read by the kernel (no
    .item()).  Returns (grad_f0 or None, grad_f1 or None) as need0 / need1 ask, laid out like the features; None
    (alone) when the kernel does not serve the shape."""
    n, c, hw = _lpips_distance_shape(f0, f1, w)
    if not (need0 or need1):
        return None, None
    gl = grad.reshape(-1)
    if gl.numel() != n:
        raise ValueError(f'lpips_distance_backward: grad must hold one element per sample ({n}), got {tuple(grad.shape)}')
    gl = gl.to(device=f0.device, dtype=torch.float32).contiguous()
    w = w.contiguous()
    p0, p1, pw, pg = fp(f0), fp(f1), fp(w), fp(gl)
    g0 = torch.empty_like(f0) if need0 else None        # preserve_format: NHWC-dense like f0
    g1 = torch.empty_like(f1) if need1 else None
    if n == 0:
        return g0, g1
    with launching(f0, 'lpips_distance', (n, c, hw, 1)) as stream:
        st = lib().fmgan_lpips_distance_backward_f32(p0, p1, pw, pg, fp(g0), fp(g1), n, c, hw, float(eps), stream)
    return (g0, g1) if served(st, 'lpips_distance_backward') else None


# ----------------------------------------------------------------------------- csrc/ppl_input.hip
def lpips_pair_input(image, shift, scale, window, f):
    """Input stage of the perceptual path length in one launch (csrc/ppl_input.hip): image [2P, 3, H, W] f32 contiguous
    (sample 2p / 2p+1: the two images of pair p), shift / scale the three floats of lpips.ScalingLayer's buffers on the
    image's device (read by the kernel), window = (y0, x0, hc, wc), f in {1, 2, 4} the bilinear reduction ->
    (in0, in1), each [P, 3, hc/f, wc/f] in channels_last storage: ((window of image[::2] / image[1::2], reduced) - shift)
    / scale.  None when the library declines (another f, a window f does not divide): the caller then evaluates the
    composite.  Tensors of another dtype, device or layout are refused (RuntimeError), as is another shape (ValueError)."""
    if image.ndim != 4 or image.shape[1] != 3 or image.shape[0] % 2 != 0 or shift.numel() != 3 or scale.numel() != 3:
        raise ValueError(f'lpips_pair_input: image {tuple(image.shape)}, shift {tuple(shift.shape)}, scale '
                         f'{tuple(scale.shape)}: expected [2P, 3, H, W] and three floats each')
    shift, scale = shift.contiguous(), scale.contiguous()
    require_f32_gpu('lpips_pair_input', ((image, 'image'), (shift, 'shift'), (scale, 'scale')))
    n, _, h, w = image.shape
    y0, x0, hc, wc = (int(v) for v in window)
    f = int(f)
    if n == 0 or lib().fmgan_lpips_pair_input_select(n // 2, h, w, y0, x0, hc, wc, f) == FMGAN_EUNSUPPORTED:
        return None
    with launching(image, 'lpips_pair_input', (n // 2, h, w, y0, x0, hc, wc, f)) as stream:
        out0 = _nhwc_empty(n // 2, 3, max(hc // f, 0), max(wc // f, 0), image.device)
        out1 = torch.empty_like(out0)
        st = lib().fmgan_lpips_pair_input_f32(fp(image), fp(shift), fp(scale), fp(out0), fp(out1), n // 2, h, w, y0, x0,
                                              hc, wc, f, stream)
    return (out0, out1) if served(st, 'lpips_pair_input') else None


# ----------------------------------------------------------------------------- csrc/projection_loss.hip
def _projection_loss_args(x, target, mask, vectors):
    """(batch, size, f) after the checks shared by the two projection-stage entry points: shapes first (ValueError), then
    device, dtype (RuntimeError from fp(), no fallback) and layout.  `vectors`: the three-float device vectors."""
    if x.ndim != 4 or x.shape[1] != 3 or tuple(target.shape) != tuple(x.shape) or \
            (mask is not None and tuple(mask.shape) != tuple(x.shape[2:])) or any(v.numel() != 3 for v in vectors):
        raise ValueError(f'projection_loss: x {tuple(x.shape)}, target {tuple(target.shape)}, mask '
                         f'{None if mask is None else tuple(mask.shape)}: expected two [B, 3, S, S] tensors, an [S, S] '
                         f'mask or none, and three floats each of shift / scale')
    require_f32_gpu('projection_loss', ((x, 'x'), (target, 'target'), (mask, 'mask')) +
                    tuple((v, 'shift / scale') for v in vectors))
    b, _, h, w = x.shape
    return b, h, w, max(h // LPIPS_SIZE, 1)


def projection_loss_fwd(x, target, mask, shift, scale, want_y=True):
    """Forward of the projection criterion's image stage in one launch (csrc/projection_loss.hip): x, target [B, 3, S, S]
    f32 contiguous, S in {256, 512, 1024}, mask [S, S] or None, shift / scale the three floats of lpips.ScalingLayer's
    buffers on x's device -> (partial, y): partial [blocks] f32, fixed-order sums of (x - target)^2 (* mask) whose total is
    the squared error (bit-reproducible; add with sum(dtype=float64)); y [B, 3, 256, 256] in channels_last storage,
    (bilinear(clamp(x, -1, 1)) - shift) / scale, or None when not wanted.  None (alone) when the library declines the
    shape: the caller then evaluates the composite."""
    b, h, w, f = _projection_loss_args(x, target, mask, (shift, scale))
    blocks = 0 if b == 0 else lib().fmgan_projection_loss_blocks(b, h, w, f)
    if blocks <= 0:
        return None
    with launching(x, 'projection_loss', (b, h, f, mask is not None, bool(want_y), 0)) as stream:
        partial = torch.empty((blocks,), dtype=torch.float32, device=x.device)
        y = _nhwc_empty(b, 3, LPIPS_SIZE, LPIPS_SIZE, x.device) if want_y else None
        st = lib().fmgan_projection_loss_fwd_f32(fp(x), fp(target), fp(mask), fp(shift), fp(scale), fp(partial), fp(y),
                                                 b, h, w, f, stream)
    return (partial, y) if served(st, 'projection_loss_fwd') else None


def projection_loss_bwd(x, target, mask, g_y, k, scale):
    """Backward of the stage in one launch: grad_x = k * (x - target) * mask + the gradient g_y [B, 3, 256, 256]
    (channels_last storage, or None) of y carried back through ScalingLayer, the bilinear reduction and the clamp.
    k: one f32 element ON THE DEVICE (grad_loss * 2 * mse_weight / denominator), read by the kernel (no .item()).
    None when the library declines the shape."""
    b, h, w, f = _projection_loss_args(x, target, mask, (scale,))
    if k.numel() != 1 or k.device != x.device:
        raise ValueError(f'projection_loss_bwd: k must hold one element on x\'s device, got {tuple(k.shape)} on {k.device}')
    if g_y is not None:
        if tuple(g_y.shape) != (b, 3, LPIPS_SIZE, LPIPS_SIZE) or not nhwc_dense(g_y) or g_y.device != x.device:
            raise ValueError(f'projection_loss_bwd: g_y {tuple(g_y.shape)} with strides {g_y.stride()}: expected '
                             f'[{b}, 3, {LPIPS_SIZE}, {LPIPS_SIZE}] in channels_last storage on x\'s device')
    pk, pg = fp(k), fp(g_y)
    if b == 0 or lib().fmgan_projection_loss_select(b, h, w, f) <= 0:
        return None
    with launching(x, 'projection_loss', (b, h, f, mask is not None, g_y is not None, 1)) as stream:
        grad_x = torch.empty_like(x)
        st = lib().fmgan_projection_loss_bwd_f32(fp(x), fp(target), fp(mask), pg, pk, fp(scale), fp(grad_x), b, h, w, f,
                                                 stream)
    return grad_x if served(st, 'projection_loss_bwd') else None


# ----------------------------------------------------------------------------- landmark stages (csrc/landmark.hip)
HEATMAP_SIZE = 64                         # the side of the alignment network's heat maps (the decode kernel's only size)


def _box_ptr(box, n, device, what):
    """data_ptr of the [n, 4] int32 box tensor on `device` (ux, uy, bx, by per sample), read by the crop kernels."""
    if tuple(box.shape) != (n, 4):
        raise ValueError(f'{what}: box {tuple(box.shape)}: expected [{n}, 4] (ux, uy, bx, by per sample)')
    if box.dtype != torch.int32 or box.device != device or not box.is_contiguous():
        raise RuntimeError(f'{what}: box must be a contiguous int32 tensor on {device}, got {box.dtype} on {box.device}')
    return box.data_ptr()


def face_crop_serves(n, h, w, r):
    """Do the crop kernels take [n, 3, h, w] images and r x r crops (host logic, nothing runs)?"""
    return n > 0 and lib().fmgan_face_crop_select(int(n), int(h), int(w), int(r)) > 0


def face_crop_fwd(img, box, r):
    """Face crop in one launch for the batch (csrc/landmark.hip): img [N, 3, H, W] f32 contiguous in [-1, 1], box [N, 4]
    int32 on img's device -> [N, 3, r, r] in [0, 1]: Get_HeatMap_PyTorch's scaling, Crop_PyTorch and the division by
    255.  None when the library declines the sizes."""
    if img.ndim != 4 or img.shape[1] != 3:
        raise ValueError(f'face_crop: img {tuple(img.shape)}: expected [N, 3, H, W]')
    require_f32_gpu('face_crop', ((img, 'img'),))
    n, _, h, w = img.shape
    r = int(r)
    pb = _box_ptr(box, n, img.device, 'face_crop')
    if not face_crop_serves(n, h, w, r):
        return None
    with launching(img, 'face_crop', (n, h, w, r, 0)) as stream:
        out = torch.empty((n, 3, r, r), dtype=torch.float32, device=img.device)
        st = lib().fmgan_face_crop_fwd_f32(fp(img), pb, fp(out), n, h, w, r, stream)
    return out if served(st, 'face_crop_fwd') else None


def face_crop_bwd(grad_out, box, h, w):
    """Gradient of face_crop_fwd with respect to img in one launch: grad_out [N, 3, r, r] f32 contiguous -> [N, 3, h, w],
    exactly 0 outside the crops, bit-reproducible (gather, fixed order).  None when the library declines the sizes."""
    if grad_out.ndim != 4 or grad_out.shape[1] != 3 or grad_out.shape[2] != grad_out.shape[3]:
        raise ValueError(f'face_crop_bwd: grad_out {tuple(grad_out.shape)}: expected [N, 3, r, r]')
    require_f32_gpu('face_crop_bwd', ((grad_out, 'grad_out'),))
    n, _, r, _ = grad_out.shape
    h, w = int(h), int(w)
    pb = _box_ptr(box, n, grad_out.device, 'face_crop_bwd')
    if not face_crop_serves(n, h, w, r):
        return None
    with launching(grad_out, 'face_crop', (n, h, w, r, 1)) as stream:
        grad_img = torch.empty((n, 3, h, w), dtype=torch.float32, device=grad_out.device)
        st = lib().fmgan_face_crop_bwd_f32(fp(grad_out), pb, fp(grad_img), n, h, w, r, stream)
    return grad_img if served(st, 'face_crop_bwd') else None


def detector_input(img):
    """The face detector's input in one launch: img [N, 3, H, W] f32 contiguous in [-1, 1] ->
    ((img + 1) * 255 / 2).flip(1) - (104, 117, 123).  None for an empty batch."""
    if img.ndim != 4 or img.shape[1] != 3:
        raise ValueError(f'detector_input: img {tuple(img.shape)}: expected [N, 3, H, W]')
    require_f32_gpu('detector_input', ((img, 'img'),))
    n, _, h, w = img.shape
    if n == 0 or h * w == 0:
        return None
    with launching(img, 'detector_input', (n, h, w)) as stream:
        out = torch.empty_like(img)
        st = lib().fmgan_detector_input_f32(fp(img), fp(out), n, h * w, stream)
    check(st, 'detector_input')
    return out


def _heatmap_distance_shape(a, b):
    if a.ndim < 2 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f'heatmap_distance: {tuple(a.shape)} and {tuple(b.shape)}: expected two [N, ...] tensors of one '
                         f'shape')
    require_f32_gpu('heatmap_distance', ((a, 'a'), (b, 'b')))
    n = a.shape[0]
    return n, (a.numel() // n if n else 0)


def heatmap_distance_serves(n, m):
    """Do the distance kernels take n samples of m elements (host logic, nothing runs)?"""
    return n > 0 and lib().fmgan_heatmap_distance_blocks(int(n), int(m)) > 0


def heatmap_distance_fwd(a, b):
    """Per-sample squared distance in one launch: a, b [N, ...] f32 contiguous of one shape -> partial [N, blocks] f32,
    fixed-order sums of (a - b)^2 over 4096 elements each (bit-reproducible; add with sum(1, dtype=float64)).  None when
    the library declines (a sample's element count no multiple of 4)."""
    n, m = _heatmap_distance_shape(a, b)
    blocks = lib().fmgan_heatmap_distance_blocks(n, m) if n else 0
    if blocks <= 0:
        return None
    with launching(a, 'heatmap_distance', (n, m, 0)) as stream:
        partial = torch.empty((n, blocks), dtype=torch.float32, device=a.device)
        st = lib().fmgan_heatmap_distance_fwd_f32(fp(a), fp(b), fp(partial), n, m, stream)
    return partial if served(st, 'heatmap_distance_fwd') else None


def heatmap_distance_bwd(a, b, grad, need_a, need_b):
    """Gradients of the distance in one launch: grad [N] f32 ON THE DEVICE is the upstream gradient, read by the kernel
    (no .item()).  Returns (grad_a or None, grad_b or None) as need_a / need_b ask; None (alone) when not served."""
    n, m = _heatmap_distance_shape(a, b)
    if not (need_a or need_b):
        return None, None
    g = grad.reshape(-1)
    if g.numel() != n:
        raise ValueError(f'heatmap_distance_bwd: grad must hold one element per sample ({n}), got {tuple(grad.shape)}')
    g = g.to(device=a.device, dtype=torch.float32).contiguous()
    if not heatmap_distance_serves(n, m):
        return None
    with launching(a, 'heatmap_distance', (n, m, 1)) as stream:
        ga = torch.empty_like(a) if need_a else None
        gb = torch.empty_like(b) if need_b else None
        st = lib().fmgan_heatmap_distance_bwd_f32(fp(a), fp(b), fp(g), fp(ga), fp(gb), n, m, stream)
    return (ga, gb) if served(st, 'heatmap_distance_bwd') else None


def landmark_decode(hm, center=None, scale=None):
    """_get_preds_fromhm_torch in one launch, one wave per map: hm [B, C, 64, 64] f32 contiguous, center [B, 2] and scale
    [B] f32 on hm's device (both or neither) -> (preds, preds_orig), each [B, C, 2].  None when the library declines
    (maps of another size)."""
    if hm.ndim != 4 or (center is None) != (scale is None) or \
            (center is not None and (tuple(center.shape) != (hm.shape[0], 2) or tuple(scale.shape) != (hm.shape[0],))):
        raise ValueError(f'landmark_decode: hm {tuple(hm.shape)}, center '
                         f'{None if center is None else tuple(center.shape)}, scale '
                         f'{None if scale is None else tuple(scale.shape)}: expected [B, C, H, W], and [B, 2] with [B] '
                         f'or neither')
    require_f32_gpu('landmark_decode', ((hm, 'hm'), (center, 'center'), (scale, 'scale')))
    b, c, h, w = hm.shape
    if b * c == 0 or (h, w) != (HEATMAP_SIZE, HEATMAP_SIZE):
        return None
    with launching(hm, 'landmark_decode', (b, c)) as stream:
        preds = torch.empty((b, c, 2), dtype=torch.float32, device=hm.device)
        preds_orig = torch.empty_like(preds)
        st = lib().fmgan_landmark_decode_f32(fp(hm), fp(center), fp(scale), fp(preds), fp(preds_orig), b, c, h, w, stream)
    return (preds, preds_orig) if served(st, 'landmark_decode') else None
