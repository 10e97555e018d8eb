"""upfirdn2d, the fused bias-activations and their 16-bit forms: csrc/upfirdn2d.hip, fused_bias_act.hip, act16.hip."""
import ctypes
import functools

import torch

from . import core
from .core import (
    ambient, amp_fwd, BF16, check, dtype_code, F16, F32, fp, launching, lib, _noise_args, on_device, ptr,
    require_gpu, served)

_DTYPES16 = {torch.float16: F16, torch.bfloat16: BF16}

# Activations of op/upfirdn2d.py and op/fused_act.py in HBM: 'fp32' (default: under autocast amp_fwd widens their 16-bit
# inputs, the fp32 kernels run and hand fp32 on) or '16' (16-bit tensors stay 16-bit on the kernels of csrc/act16.hip:
# half the bytes and no cast kernels around each op; f16 takes those kernels too).  bf16 tensors outside autocast run on
# the 16-bit kernels in either mode; f16 tensors in 'fp32' mode keep the generic kernels.  Context manager only.
_act_io = 'fp32'


class activation_io(ambient):
    """`with activation_io('16'):` — inside, and under torch.autocast, FusedLeakyReLU / fused_leaky_relu / Blur / upfirdn2d
    keep a 16-bit input 16-bit (fp32 inputs stay on the fp32 kernels)."""
    values, text, scope, var = ('fp32', '16'), "mode must be 'fp32' or '16'", globals(), '_act_io'


def current_activation_io():
    return _act_io


def io16(t):
    """Does this tensor run on the 16-bit kernels (act16.hip)?  bf16 always; f16 under activation_io('16')."""
    return t.dtype == torch.bfloat16 or (t.dtype == torch.float16 and _act_io == '16')


def amp_fwd_io(fwd):
    """amp_fwd for the Functions of op/upfirdn2d.py and op/fused_act.py: under autocast and activation_io('16') the
    forward runs with autocast off and its inputs AS THEY ARE (nothing is widened; an fp32 input stays on the fp32
    kernels), and amp_bwd runs the backward the same way; otherwise exactly amp_fwd."""
    cast = amp_fwd(fwd)

    @functools.wraps(fwd)
    def decorate(ctx, *args, **kwargs):
        if _act_io == '16' and torch.is_autocast_enabled('cuda'):
            ctx._dtype = torch.get_autocast_dtype('cuda')
            ctx._fwd_used_autocast = False
            with torch.autocast(device_type='cuda', enabled=False):
                return fwd(ctx, *args, **kwargs)
        return cast(ctx, *args, **kwargs)

    return decorate


# ----------------------------------------------------------------------------- csrc/upfirdn2d.hip
BLUR_PATHS = {}      # (planes, in_h, in_w) -> kernel id of the last fused blur of that shape, while an observer asks


def upfirdn2d_out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    oh, ow = ctypes.c_int(), ctypes.c_int()
    check(lib().fmgan_upfirdn2d_out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1,
                                         ctypes.byref(oh), ctypes.byref(ow)), 'upfirdn2d_out_size')
    return oh.value, ow.value


def upfirdn2d(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1, force_path=-1):
    """Same positional signature and layout as the reference's pybind `upfirdn2d` (op/upfirdn2d.cpp:12-23):
    input [major,in_h,in_w,minor], kernel [kh,kw] -> new tensor [major,out_h,out_w,minor]."""
    require_gpu(input, 'input')
    require_gpu(kernel, 'kernel')
    if force_path == -1 and io16(input):
        return upfirdn2d16(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
    x = input.contiguous()
    k = kernel.to(dtype=x.dtype).contiguous()
    major, in_h, in_w, minor = x.shape
    kh, kw = k.shape
    out_h, out_w = upfirdn2d_out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
    if out_h <= 0 or out_w <= 0:
        raise RuntimeError(f'upfirdn2d: empty output {out_h}x{out_w}')
    out = torch.empty((major, out_h, out_w, minor), dtype=x.dtype, device=x.device)
    with launching(x, 'upfirdn2d', (major, in_h, in_w, out_h, out_w, up_x, down_x, x.element_size())) as stream:
        st = lib().fmgan_upfirdn2d(dtype_code(x), ptr(x), ptr(k), ptr(out), major, in_h, in_w, minor, kh, kw,
                                   up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1, force_path, stream)
    check(st, 'upfirdn2d')
    return out


def upfirdn2d_strided(in_ptr, device, major, in_h, in_w, plane_stride, row_stride, kernel, pad_x0, pad_x1, pad_y0, pad_y1,
                      force_path=-1):
    """up=down=1 FIR of a strided f32 input [major, in_h, in_w] (see aligned_rows_buffer) -> contiguous [major,out_h,out_w].
    force_path: -1 automatic; 4 = register row-march (path 1), 5 = LDS-DMA ring (path 1b) — A/B tests only."""
    k = kernel.contiguous()
    kh, kw = k.shape
    out_h, out_w = upfirdn2d_out_size(in_h, in_w, kh, kw, 1, 1, 1, 1, pad_x0, pad_x1, pad_y0, pad_y1)
    out = torch.empty((major, out_h, out_w), dtype=torch.float32, device=device)
    with launching(out, 'upfirdn2d', (major, in_h, in_w, out_h, out_w, 1, 1, 4)) as stream:
        st = lib().fmgan_upfirdn2d_strided(F32, in_ptr, fp(k), fp(out), major, in_h, in_w, 1, plane_stride, row_stride,
                                           kh, kw, 1, 1, 1, 1, pad_x0, pad_x1, pad_y0, pad_y1, force_path, stream)
    check(st, 'upfirdn2d_strided')
    return out


def blur_noise_bias_act_serves(batch, channels, in_h, in_w, plane_stride, row_stride, kernel_shape, pad):
    """Would blur_noise_bias_act launch a kernel for this shape (host logic, nothing runs)?  False is the case in which
    it returns None: neither the row-march nor the plane-tile kernel serves the plane size or a FIR wider than 4 taps."""
    kh, kw = kernel_shape
    pad0, pad1 = pad
    return lib().fmgan_blur_noise_bias_act_select(None, None, None, batch, channels, in_h, in_w, plane_stride, row_stride,
                                                  kh, kw, pad0, pad1, pad0, pad1) > 0


def blur_noise_bias_act(in_ptr, device, batch, channels, in_h, in_w, plane_stride, row_stride, kernel, pad, noise,
                        noise_weight, bias, alpha, scale, force_path=-1, out=None):
    """blur -> (+noise) -> +bias -> lrelu*scale in one pass over a strided f32 input; returns [B,C,out_h,out_w] or None
    when neither the row-march kernels (out_w >= 64) nor the plane-tile kernel (planes up to ~110^2) serve the shape
    (the caller then uses the two-pass form)."""
    k = kernel.contiguous()
    kh, kw = k.shape
    pad0, pad1 = pad
    out_h, out_w = upfirdn2d_out_size(in_h, in_w, kh, kw, 1, 1, 1, 1, pad0, pad1, pad0, pad1)
    if out_w <= 0 or out_h <= 0:
        return None
    if out is None:
        out = torch.empty((batch, channels, out_h, out_w), dtype=torch.float32, device=device)
    elif tuple(out.shape) != (batch, channels, out_h, out_w) or not out.is_contiguous() or out.dtype != torch.float32:
        raise RuntimeError('blur_noise_bias_act: `out` must be a contiguous f32 [B,C,out_h,out_w] tensor')
    nz, nb = _noise_args(noise)
    if getattr(core._observer, 'wants_paths', False):     # through its owner: set_observer rebinds it
        BLUR_PATHS[(batch * channels, in_h, in_w)] = lib().fmgan_blur_noise_bias_act_select(
            in_ptr, fp(out), fp(nz), batch, channels, in_h, in_w, plane_stride, row_stride, kh, kw, pad0, pad1, pad0, pad1)
    with launching(out, 'upfirdn2d', (batch * channels, in_h, in_w, out_h, out_w, 1, 1, 4)) as stream:
        st = lib().fmgan_blur_noise_bias_act_path_f32(in_ptr, fp(k), fp(out), batch, channels, in_h, in_w,
                                                      plane_stride, row_stride, kh, kw, pad0, pad1, pad0, pad1, fp(nz),
                                                      fp(noise_weight), fp(bias), nb, float(alpha), float(scale),
                                                      force_path, stream)
    return out if served(st, 'blur_noise_bias_act') else None


# ----------------------------------------------------------------------------- csrc/fused_bias_act.hip
def fused_bias_act(input, bias, refer, act, grad, alpha, scale):
    """Same positional signature as the reference's pybind `fused_bias_act` (op/fused_bias_act.cpp:11-21);
    empty `bias` / `refer` tensors mean "absent" (op/fused_bias_act_kernel.cu:62-63)."""
    require_gpu(input, 'input')
    if bias is not None and bias.numel():
        require_gpu(bias, 'bias')
    if io16(input):
        return fused_bias_act16(input, bias, refer, act, grad, alpha, scale)
    x = input.contiguous()
    b = bias.to(dtype=x.dtype).contiguous() if bias is not None and bias.numel() else None
    r = refer.to(dtype=x.dtype).contiguous() if refer is not None and refer.numel() else None
    if r is not None and r.numel() != x.numel():
        raise RuntimeError('fused_bias_act: refer must have as many elements as input')
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    out = torch.empty_like(x)
    with launching(x, 'fused_bias_act', (x.numel(), x.element_size())) as stream:
        st = lib().fmgan_fused_bias_act(dtype_code(x), ptr(x), ptr(b), ptr(r), ptr(out), x.numel(),
                                        0 if b is None else b.numel(), step_b, int(act), int(grad), float(alpha),
                                        float(scale), stream)
    check(st, 'fused_bias_act')
    return out


def fused_bias_act_backward(grad_output, out, alpha, scale):
    """grad_input of lrelu(x + b) * scale AND the bias gradient from ONE pass over the data: returns
    (grad_input, grad_bias [C]) or None when the kernel does not serve the shape (not f32, < 3 dims, planes of fewer
    than 64 or not a multiple of 4 elements) — the caller then runs fused_bias_act(..., 3, 1) and a torch sum."""
    require_gpu(grad_output, 'input')
    if grad_output.dtype != torch.float32 or grad_output.ndim < 3 or out.dtype != torch.float32:
        return None
    g = grad_output.contiguous()
    r = out.contiguous()
    b, c = g.shape[:2]
    hw = g[0, 0].numel()
    gx = lib().fmgan_fused_bias_act_bwd_blocks(b * c, hw)
    if gx == 0 or r.numel() != g.numel():
        return None
    gi = torch.empty_like(g)
    partial = torch.empty((b, c, gx), dtype=torch.float32, device=g.device)
    with launching(g, 'fused_bias_act', (g.numel(), 4)) as stream:
        st = lib().fmgan_fused_bias_act_bwd_f32(fp(g), fp(r), fp(gi), fp(partial), b * c, hw, float(alpha),
                                                float(scale), stream)
    return (gi, partial.sum((0, 2))) if served(st, 'fused_bias_act_backward') else None


def noise_bias_act(x, noise, noise_weight, bias, alpha, scale):
    """lrelu(x + noise_weight*noise + bias[c]) * scale in one pass; x [B,C,H,W] f32, noise [1|B,1,H,W]."""
    require_gpu(x, 'input')
    x = x.contiguous()
    b, c, h, w = x.shape
    nz, nb = _noise_args(noise)
    out = torch.empty_like(x)
    with launching(x, 'noise_bias_act', (x.numel(), 4)) as stream:
        st = lib().fmgan_noise_bias_act_f32(fp(x), fp(nz), fp(noise_weight), fp(bias), fp(out), b, c, h * w, nb,
                                            float(alpha), float(scale), stream)
    check(st, 'noise_bias_act')
    return out


def prelu_backward(x, grad, slope):
    """Backward of PReLU on channels-innermost data: x, grad [rows, C] f32 contiguous, slope [C] ->
    (grad_x [rows, C], grad_slope [C]).  Returns None when the kernel does not serve the shape (C % 4 != 0)."""
    require_gpu(x, 'input')
    rows, c = x.shape
    if c % 4 != 0 or rows == 0:
        return None
    blocks = lib().fmgan_prelu_backward_blocks(rows, c)
    gx = torch.empty_like(x)
    partial = torch.empty((blocks, c), dtype=torch.float32, device=x.device)
    with on_device(x) as stream:
        st = lib().fmgan_prelu_backward_f32(fp(x), fp(grad), fp(slope), fp(gx), fp(partial), rows, c, stream)
    return (gx, partial.sum(0)) if served(st, 'prelu_backward') else None


# ----------------------------------------------------------------------------- 16-bit activations (csrc/act16.hip)
def dtype16_code(t):
    try:
        return _DTYPES16[t.dtype]
    except KeyError:
        raise RuntimeError(f'unsupported dtype {t.dtype}: the 16-bit kernels take float16/bfloat16 only') from None


def _same_device(what, x, named):
    for t, name in named:
        if t is not None and t.device != x.device:
            raise RuntimeError(f'{what}: {name} is on {t.device}, input on {x.device}')


def upfirdn2d16(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """upfirdn2d on a bf16 / f16 tensor [major,in_h,in_w,minor] without widening it: the taps are read as fp32 (a 16-bit
    `kernel` of a converted module is widened here, which is exact), the sums are fp32 and the result is rounded once."""
    require_gpu(input, 'input')
    require_gpu(kernel, 'kernel')
    _same_device('upfirdn2d', input, ((kernel, 'kernel'),))
    x = input.contiguous()
    k = kernel.to(dtype=torch.float32).contiguous()
    major, in_h, in_w, minor = x.shape
    kh, kw = k.shape
    out_h, out_w = upfirdn2d_out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
    if out_h <= 0 or out_w <= 0:
        raise RuntimeError(f'upfirdn2d: empty output {out_h}x{out_w}')
    out = torch.empty((major, out_h, out_w, minor), dtype=x.dtype, device=x.device)
    with launching(x, 'upfirdn2d', (major, in_h, in_w, out_h, out_w, up_x, down_x, x.element_size())) as stream:
        st = lib().fmgan_ufd16(dtype16_code(x), ptr(x), fp(k), ptr(out), major, in_h, in_w, minor, kh, kw, up_x, up_y,
                               down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1, stream)
    check(st, 'upfirdn2d16')
    return out


def fused_bias_act16(input, bias, refer, act, grad, alpha, scale):
    """fused_bias_act on a bf16 / f16 tensor without widening it; the bias is handed over as fp32 (a parameter under
    autocast is fp32 already; a 16-bit bias of a converted module is widened here, which is exact)."""
    require_gpu(input, 'input')
    x = input.contiguous()
    b = bias.to(dtype=torch.float32).contiguous() if bias is not None and bias.numel() else None
    r = refer.to(dtype=x.dtype).contiguous() if refer is not None and refer.numel() else None
    if b is not None:
        require_gpu(b, 'bias')
    _same_device('fused_bias_act', x, ((b, 'bias'), (r, 'refer')))
    if r is not None and r.numel() != x.numel():
        raise RuntimeError('fused_bias_act: refer must have as many elements as input')
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    out = torch.empty_like(x)
    with launching(x, 'fused_bias_act', (x.numel(), x.element_size())) as stream:
        st = lib().fmgan_act16_fba(dtype16_code(x), ptr(x), fp(b), ptr(r), ptr(out), x.numel(),
                                   0 if b is None else b.numel(), step_b, int(act), int(grad), float(alpha),
                                   float(scale), stream)
    check(st, 'fused_bias_act16')
    return out


# act16_fba_bwd gives every (batch, channel) plane a row of 256-thread blocks.  Below one wave of elements per plane —
# the [B, C] tensors of EqualLinear(fused_lrelu) are planes of ONE element — that is a block per handful of elements:
# such tensors take the elementwise kernel over the whole tensor and one fp32 torch sum of the stored 16-bit gradient.
_BWD16_MIN_HW = 64


def fused_bias_act16_backward(grad_output, out, alpha, scale):
    """fused_bias_act_backward on bf16 / f16 tensors of at least 2 dims: (grad_input in the tensors' dtype, grad_bias
    [C] in fp32 — the sum of the stored grad_input), or None for a tensor of fewer dims or mixed dtypes (the caller then
    runs fused_bias_act(..., 3, 1) and a torch sum)."""
    require_gpu(grad_output, 'input')
    if (grad_output.ndim < 2 or grad_output.numel() == 0 or out.dtype != grad_output.dtype
            or out.numel() != grad_output.numel()):
        return None
    _same_device('fused_bias_act_backward', grad_output, ((out, 'out'),))
    g = grad_output.contiguous()
    r = out.contiguous()
    b, c = g.shape[:2]
    hw = g[0, 0].numel()
    if hw < _BWD16_MIN_HW:
        gi = fused_bias_act16(g, None, r, 3, 1, alpha, scale)
        return gi, gi.sum([0] + list(range(2, g.ndim)), dtype=torch.float32)
    gx = lib().fmgan_act16_fba_bwd_blocks(b * c, hw)
    if gx == 0:
        return None
    gi = torch.empty_like(g)
    partial = torch.empty((b, c, gx), dtype=torch.float32, device=g.device)
    with launching(g, 'fused_bias_act', (g.numel(), g.element_size())) as stream:
        st = lib().fmgan_act16_fba_bwd(dtype16_code(g), ptr(g), ptr(r), ptr(gi), fp(partial), b * c, hw, float(alpha),
                                       float(scale), stream)
    check(st, 'fused_bias_act16_backward')
    return gi, partial.sum((0, 2))
