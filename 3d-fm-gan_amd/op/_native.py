"""ctypes binding of libfmgan_hip.so (include/fmgan_hip.h) — the only way the host code reaches a kernel.

There is NO fallback: if the library is missing, or a tensor is not on the GPU, this raises.
PyTorch is used for device memory and streams only; every launch goes on torch's current HIP stream
of the tensor's device (as the reference launches on at::cuda::getCurrentCUDAStream,
op/upfirdn2d_kernel.cu:213-215), asynchronously, so calls can be captured in a HIP graph.
"""
import ctypes
import functools
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('FMGAN_LIB') or os.path.join(os.path.dirname(_HERE), 'csrc', 'libfmgan_hip.so')

F32, F64, F16 = 0, 1, 2
BF16 = 3                                  # the 16-bit activation kernels only (csrc/act16.hip)
FMGAN_OK, FMGAN_EINVAL, FMGAN_EUNSUPPORTED = 0, -1, -2      # include/fmgan_hip.h, status codes
LPIPS_SIZE = 256                          # the size LPIPS is evaluated at (TARGET of op.ppl_input, op.projection_loss)
_DTYPES = {torch.float32: F32, torch.float64: F64, torch.float16: F16}
_DTYPES16 = {torch.float16: F16, torch.bfloat16: BF16}

_lib = None

# Under torch.autocast (BASELINE config 5's bf16 leg) the MIOpen convolutions hand bf16 tensors to their consumers; the
# HIP kernels compute in fp32 (their reference counterparts dispatch float / double / half only): every custom autograd
# Function of this package is entered with autocast off and its floating-point CUDA inputs cast to fp32.  A no-op when
# autocast is not active.
amp_fwd = torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
amp_bwd = torch.amp.custom_bwd(device_type='cuda')

# Activations of op/upfirdn2d.py and op/fused_act.py in HBM: 'fp32' (default: under autocast amp_fwd widens their 16-bit
# inputs, the fp32 kernels run and hand fp32 on) or '16' (16-bit tensors stay 16-bit on the kernels of csrc/act16.hip:
# half the bytes and no cast kernels around each op; f16 takes those kernels too).  bf16 tensors outside autocast run on
# the 16-bit kernels in either mode; f16 tensors in 'fp32' mode keep the generic kernels.  Context manager only.
_act_io = 'fp32'


class activation_io:
    """`with activation_io('16'):` — inside, and under torch.autocast, FusedLeakyReLU / fused_leaky_relu / Blur / upfirdn2d
    keep a 16-bit input 16-bit (fp32 inputs stay on the fp32 kernels)."""

    def __init__(self, mode):
        if mode not in ('fp32', '16'):
            raise ValueError("mode must be 'fp32' or '16'")
        self.mode = mode

    def __enter__(self):
        global _act_io
        self.prev, _act_io = _act_io, self.mode
        return self

    def __exit__(self, *exc):
        global _act_io
        _act_io = self.prev
        return False


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


def _sig(fn, argtypes, restype=ctypes.c_int):
    fn.argtypes = argtypes
    fn.restype = restype
    return fn


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} not found: the HIP extension is not built. Run `make -C {os.path.dirname(LIB_PATH)}` '
            f'(or __graft_entry__.build()). There is no CPU or PyTorch fallback for these ops.')
    L = ctypes.CDLL(LIB_PATH)
    vp, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    _sig(L.fmgan_abi_version, [])
    _sig(L.fmgan_status_string, [i], ctypes.c_char_p)
    _sig(L.fmgan_upfirdn2d_select, [i] * 15)
    _sig(L.fmgan_upfirdn2d_out_size, [i] * 12 + [ctypes.POINTER(i)] * 2)
    _sig(L.fmgan_upfirdn2d, [i, vp, vp, vp] + [i] * 15 + [vp])
    _sig(L.fmgan_upfirdn2d_strided, [i, vp, vp, vp] + [i] * 4 + [ll, i] + [i] * 11 + [vp])
    _sig(L.fmgan_blur_noise_bias_act_f32, [vp] * 3 + [i] * 4 + [ll, i] + [i] * 6 + [vp] * 3 + [i, f, f, vp])
    _sig(L.fmgan_blur_noise_bias_act_select, [vp] * 3 + [i] * 4 + [ll, i] + [i] * 6)
    _sig(L.fmgan_blur_noise_bias_act_path_f32, [vp] * 3 + [i] * 4 + [ll, i] + [i] * 6 + [vp] * 3 + [i, f, f, i, vp])
    _sig(L.fmgan_fused_bias_act, [i, vp, vp, vp, vp, ll, i, i, i, i, f, f, vp])
    _sig(L.fmgan_noise_bias_act_f32, [vp] * 5 + [i] * 4 + [f, f, vp])
    _sig(L.fmgan_fused_bias_act_bwd_blocks, [ll, i])
    _sig(L.fmgan_fused_bias_act_bwd_f32, [vp] * 4 + [ll, i, f, f, vp])
    _sig(L.fmgan_prelu_backward_blocks, [ll, i])
    _sig(L.fmgan_prelu_backward_f32, [vp] * 5 + [ll, i, vp])
    _sig(L.fmgan_face_region_blocks, [i, ll])
    _sig(L.fmgan_face_region_loss_f32, [vp] * 3 + [i, i, ll, vp])
    _sig(L.fmgan_face_region_backward_f32, [vp] * 4 + [i, i, ll, vp])
    _sig(L.fmgan_render_mask_f32, [vp] * 2 + [i, i, ll, vp])
    _sig(L.fmgan_face_input_blocks, [i] * 4)
    _sig(L.fmgan_face_input_f32, [vp] * 5 + [i] * 4 + [vp])
    _sig(L.fmgan_lpips_pair_input_select, [i] * 8)
    _sig(L.fmgan_lpips_pair_input_f32, [vp] * 5 + [i] * 8 + [vp])
    _sig(L.fmgan_projection_loss_select, [i] * 4)
    _sig(L.fmgan_projection_loss_blocks, [i] * 4)
    _sig(L.fmgan_projection_loss_fwd_f32, [vp] * 7 + [i] * 4 + [vp])
    _sig(L.fmgan_projection_loss_bwd_f32, [vp] * 7 + [i] * 4 + [vp])
    _sig(L.fmgan_fid_stats_select, [i] * 2)
    _sig(L.fmgan_fid_stats_update_f32, [vp] * 4 + [i, i, vp])
    _sig(L.fmgan_fid_stats_finish_f64, [vp] * 3 + [ll, vp, vp, i, vp])
    _sig(L.fmgan_inception_input_select, [i] * 3)
    _sig(L.fmgan_inception_input_f32, [vp, vp] + [i] * 4 + [vp])
    _sig(L.fmgan_face_crop_select, [i] * 4)
    _sig(L.fmgan_face_crop_fwd_f32, [vp] * 3 + [i] * 4 + [vp])
    _sig(L.fmgan_face_crop_bwd_f32, [vp] * 3 + [i] * 4 + [vp])
    _sig(L.fmgan_detector_input_f32, [vp, vp, i, ll, vp])
    _sig(L.fmgan_heatmap_distance_blocks, [i, ll])
    _sig(L.fmgan_heatmap_distance_fwd_f32, [vp] * 3 + [i, ll, vp])
    _sig(L.fmgan_heatmap_distance_bwd_f32, [vp] * 5 + [i, ll, vp])
    _sig(L.fmgan_landmark_decode_f32, [vp] * 5 + [i] * 4 + [vp])
    _sig(L.fmgan_lpips_distance_blocks, [i] * 3)
    _sig(L.fmgan_lpips_distance_f32, [vp] * 4 + [i, i, i, f, vp])
    _sig(L.fmgan_lpips_distance_backward_f32, [vp] * 6 + [i, i, i, f, vp])
    _sig(L.fmgan_bn_prelu_f32, [vp] * 5 + [f, vp, vp] + [vp] * 4 + [f, vp, vp] + [i] * 5 + [vp])
    _sig(L.fmgan_se_pool_chunks, [i] * 4)
    _sig(L.fmgan_se_pool_f32, [vp, vp] + [i] * 4 + [vp])
    _sig(L.fmgan_se_gate_f32, [vp, i, ll] + [vp] * 4 + [f] + [vp] * 3 + [i] * 3 + [vp])
    _sig(L.fmgan_ir_tail_f32, [vp] * 5 + [f, vp, vp] + [i] * 3 + [vp] * 4 + [f, vp] + [vp] * 4 + [f, vp] + [i] * 4 + [vp])
    _sig(L.fmgan_modconv_demod_f32, [vp] * 3 + [i] * 4 + [f, f, vp])
    _sig(L.fmgan_modconv_wsq_f32, [vp] * 2 + [i] * 3 + [vp])
    _sig(L.fmgan_modconv_demod_wsq_f32, [vp] * 3 + [i] * 3 + [f, f, vp])
    _sig(L.fmgan_equal_linear_f32, [vp] * 4 + [i] * 3 + [vp])
    _sig(L.fmgan_wino_weight_f32, [vp, vp, i, i, vp])
    _sig(L.fmgan_wino_input_f32, [vp] * 3 + [i] * 4 + [vp])
    _sig(L.fmgan_wino_output_f32, [vp] * 6 + [i] * 6 + [f, f, vp])
    _sig(L.fmgan_modconv_weight_prep_f32, [vp, vp, i, i, i, f, i, vp])
    _sig(L.fmgan_modconv2d_workspace_bytes, [i] * 6, ll)
    _sig(L.fmgan_modconv2d_f32, [vp] * 5 + [i] * 6 + [vp] * 3 + [i, i, f, f, ll, i, vp, ll, vp])
    _sig(L.fmgan_modconv_weight_bf16_bytes, [i] * 3, ll)
    _sig(L.fmgan_modconv_weight_to_bf16, [vp, vp, i, i, i, vp])
    _sig(L.fmgan_modconv2d_bf16_supported, [i] * 6)
    _sig(L.fmgan_modconv2d_bf16, [vp] * 5 + [i] * 6 + [vp] * 3 + [i, i, f, f, ll, i, vp])
    _sig(L.fmgan_modconv_weight_bf16x3_bytes, [i] * 3, ll)
    _sig(L.fmgan_modconv_weight_to_bf16x3, [vp, vp, i, i, i, vp])
    _sig(L.fmgan_modconv2d_bf16x3_supported, [i] * 6)
    _sig(L.fmgan_modconv2d_bf16x3, [vp] * 5 + [i] * 6 + [vp] * 3 + [i, i, f, f, ll, i, vp])
    _sig(L.fmgan_conv3x3s2_bf16x3_supported, [i] * 5)
    _sig(L.fmgan_conv3x3s2_bf16x3_f32, [vp] * 4 + [i] * 5 + [f, i, vp])
    _sig(L.fmgan_modconv2d_rgb_fusable, [i] * 5)
    _sig(L.fmgan_modconv2d_select, [i] * 8 + [ctypes.POINTER(i)] * 5)
    _sig(L.fmgan_modconv2d_tiles, [ctypes.POINTER(i), i])
    _sig(L.fmgan_torgb_weight_mod_f32, [vp] * 3 + [i] * 3 + [f, vp])
    _sig(L.fmgan_modconv2d_rgb_f32, [vp] * 5 + [i] * 5 + [vp] * 3 + [i, i, f, f] + [vp] * 4 + [i, vp])
    _sig(L.fmgan_modconv_wgrad_workspace_bytes, [i] * 5, ll)
    _sig(L.fmgan_modconv_wgrad_f32, [vp] * 5 + [i] * 5 + [f, vp, ll, vp])
    _sig(L.fmgan_modconv_wgrad_mode_workspace_bytes, [i] * 6, ll)
    _sig(L.fmgan_modconv_wgrad_mode_f32, [vp] * 5 + [i] * 6 + [f, vp, ll, vp])
    _sig(L.fmgan_images_to_tensor, [vp, vp, i, i, i, f, f, vp])
    _sig(L.fmgan_resize_output_size, [i, i, i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)])
    _sig(L.fmgan_resize_plan_ints, [i] * 4, ll)
    _sig(L.fmgan_resize_plan, [i] * 4 + [vp, ll])
    _sig(L.fmgan_resize_bilinear_u8, [vp] * 4 + [i] * 5 + [f, f, vp])
    _sig(L.fmgan_tensor_to_images, [vp, vp, i, i, i, f, f, vp])
    _sig(L.fmgan_tiles_to_canvas, [vp, vp, ctypes.POINTER(i)] + [i] * 6 + [f, f, vp])
    _sig(L.fmgan_bank_gather, [vp] * 4 + [i] * 6 + [vp, ll, vp, ll, ll, i, i, ctypes.POINTER(i), i, vp, f, f, i, vp])
    _sig(L.fmgan_torgb_f32, [vp] * 6 + [i] * 4 + [f, vp])
    _sig(L.fmgan_torgb_backward_splits, [i] * 3)
    _sig(L.fmgan_torgb_backward_f32, [vp] * 6 + [i] * 4 + [f, vp])
    _sig(L.fmgan_refresh_entry_bytes, [])
    _sig(L.fmgan_weight_refresh_blocks, [i, i, i, i, ll], ll)
    _sig(L.fmgan_weight_refresh_f32, [vp, i, ll, vp])
    _sig(L.fmgan_style_bank_entry_bytes, [])
    _sig(L.fmgan_style_bank_f32, [vp, i, vp, vp, i, i, i, vp, vp])
    _sig(L.fmgan_demod_bank_f32, [vp, i, vp, i, vp, vp])
    _sig(L.fmgan_lbfgs_pair_blocks, [ll], ll)
    _sig(L.fmgan_lbfgs_pair_f32, [vp, i] + [vp] * 7 + [ll, i, f, i, vp])
    _sig(L.fmgan_lbfgs_coeffs_f64, [vp] * 5 + [ll, i, f, f, i, vp])
    _sig(L.fmgan_lbfgs_direction_f32, [vp] * 9 + [ll, i, vp])
    _sig(L.fmgan_lbfgs_update_f32, [vp, i, vp, f, ll, vp])
    _sig(L.fmgan_lbfgs_gather_f32, [vp, i] + [vp] * 4 + [ll, vp])
    _sig(L.fmgan_ema_blocks, [ll], ll)
    _sig(L.fmgan_ema_f32, [vp, i, ll, f, f, vp])
    _sig(L.fmgan_loss_row_f32, [vp, i, vp, vp])
    _sig(L.fmgan_act16_fba_select, [i, ll, i, i, i, i])
    _sig(L.fmgan_act16_fba, [i, vp, vp, vp, vp, ll, i, i, i, i, f, f, vp])
    _sig(L.fmgan_act16_fba_bwd_blocks, [ll, i])
    _sig(L.fmgan_act16_fba_bwd, [i] + [vp] * 4 + [ll, i, f, f, vp])
    _sig(L.fmgan_ufd16_select, [i] * 15)
    _sig(L.fmgan_ufd16, [i, vp, vp, vp] + [i] * 14 + [vp])
    if L.fmgan_abi_version() != 1:
        raise RuntimeError('libfmgan_hip.so ABI version mismatch')
    _lib = L
    return L


def check(status, what):
    if status != FMGAN_OK:
        raise RuntimeError(f'{what}: {lib().fmgan_status_string(status).decode()} (status {status})')


def served(status, what):
    """Did the library serve the launch?  False when it declined the shape (FMGAN_EUNSUPPORTED: the wrapper returns None
    and its caller takes the composite form); any other failure raises as check() does."""
    if status == FMGAN_EUNSUPPORTED:
        return False
    check(status, what)
    return True


def require_gpu(t, name):
    # op/upfirdn2d.cpp:8 CHECK_CUDA — same exception type (RuntimeError) and wording
    if not t.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA tensor (this build has no CPU path)')


def dtype_code(t):
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise RuntimeError(f'unsupported dtype {t.dtype}: float32/float64/float16 only') from None


def ptr(t):
    return None if t is None else t.data_ptr()


def fp(t):
    """data_ptr of an optional float32 GPU tensor.  The f32 entry points take raw pointers: a tensor of another dtype
    (a bf16 style vector under torch.autocast, a float64 gradcheck input) would be read past its end on the device — it is
    refused here, on the host, as a RuntimeError."""
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_cuda:
        raise RuntimeError(f'libfmgan_hip f32 entry point got a {t.dtype} tensor on {t.device}: float32 GPU tensors only '
                           f'(cast before the call; under autocast the package\'s autograd Functions do)')
    return t.data_ptr()


def require_f32_gpu(what, named, contiguous=True, same_device=True):
    """The device and dtype checks of the stage wrappers, made after their own shape test: every tensor of `named`
    ((tensor or None, name) pairs) is a float32 GPU tensor (RuntimeError from require_gpu / fp(), no fallback), and,
    unless switched off, contiguous and on the device of the first one."""
    first = None
    for t, name in named:
        if t is None:
            continue
        require_gpu(t, name)
        fp(t)
        if contiguous and not t.is_contiguous():
            raise RuntimeError(f'{what}: {name} must be contiguous, got strides {t.stride()}')
        if first is None:
            first = (t.device, name)
        elif same_device and t.device != first[0]:
            raise RuntimeError(f'{what}: {name} must be on {first[1]}\'s device')


class on_device:
    """Make the tensor's device current for the launch and hand out its current stream."""

    def __init__(self, t):
        self.dev = t.device
        self.guard = None

    def __enter__(self):
        if torch.cuda.current_device() != self.dev.index:
            self.guard = torch.cuda.device(self.dev)
            self.guard.__enter__()
        return torch.cuda.current_stream(self.dev).cuda_stream

    def __exit__(self, *exc):
        if self.guard is not None:
            self.guard.__exit__(*exc)
        return False


# ----------------------------------------------------------------------------- launch observer (bench.py)
BLUR_PATHS = {}      # (planes, in_h, in_w) -> kernel id of the last fused blur of that shape, while an observer asks


class _NullObserver:
    """bench.py installs an observer that brackets selected launches with HIP events on the launch stream."""
    wants_paths = False

    def begin(self, name, info):
        return None

    def end(self, token):
        pass


_observer = _NullObserver()


def set_observer(obs=None):
    global _observer
    _observer = obs if obs is not None else _NullObserver()


class launching(on_device):
    """on_device with the observer's bracket inside it: `with launching(t, name, info) as stream:` makes t's device
    current, then observer.begin(name, info); the block launches on `stream` and keeps each status; on leaving,
    observer.end, then the device guard is released — and only then the wrapper interprets the status (check / served).
    A block that raises releases the guard and leaves the bracket open."""

    def __init__(self, t, name, info):
        on_device.__init__(self, t)
        self.name, self.info = name, info

    def __enter__(self):
        stream = on_device.__enter__(self)
        self.tok = _observer.begin(self.name, self.info)
        return stream

    def __exit__(self, *exc):
        if exc[0] is None:
            _observer.end(self.tok)
        return on_device.__exit__(self, *exc)


def _noise_args(noise):
    """The noise argument pair of the entry points: (contiguous noise or None, its batch — 1 when there is none)."""
    if noise is None:
        return None, 1
    nz = noise.contiguous()
    return nz, nz.shape[0]


# ----------------------------------------------------------------------------- raw ops (no autograd)
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
    if getattr(_observer, 'wants_paths', False):
        BLUR_PATHS[(batch * channels, in_h, in_w)] = lib().fmgan_blur_noise_bias_act_select(
            in_ptr, fp(out), fp(nz), batch, channels, in_h, in_w, plane_stride, row_stride, kh, kw, pad0, pad1, pad0, pad1)
    with launching(out, 'upfirdn2d', (batch * channels, in_h, in_w, out_h, out_w, 1, 1, 4)) as stream:
        st = lib().fmgan_blur_noise_bias_act_path_f32(in_ptr, fp(k), fp(out), batch, channels, in_h, in_w,
                                                      plane_stride, row_stride, kh, kw, pad0, pad1, pad0, pad1, fp(nz),
                                                      fp(noise_weight), fp(bias), nb, float(alpha), float(scale),
                                                      force_path, stream)
    return out if served(st, 'blur_noise_bias_act') else None


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


def nhwc_dense(t):
    """Is the [N, C, H, W] tensor stored as one dense [N, H, W, C] block (channels_last with nothing between pixels)?"""
    return t.ndim == 4 and t.permute(0, 2, 3, 1).is_contiguous()


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


# ----------------------------------------------------------------------------- pSp encoder glue (inference)
def _nhwc(t, name):
    """(B, C, H, W) of a [B,C,H,W] f32 GPU tensor whose storage is NHWC-dense."""
    require_gpu(t, name)
    fp(t)
    if not nhwc_dense(t):
        raise RuntimeError(f'{name}: expected a [B,C,H,W] tensor in channels_last storage, got {tuple(t.shape)} with '
                           f'strides {t.stride()}')
    return tuple(t.shape)


def _bn_args(bn, c):
    """The five BatchNorm arguments of the entry points from (mean, var, gamma, beta, eps); None: five nulls."""
    if bn is None:
        return None, None, None, None, 0.0
    mean, var, gamma, beta, eps = bn
    vs = [v.contiguous() for v in (mean, var, gamma, beta)]
    if any(v.numel() != c for v in vs):
        raise ValueError(f'BatchNorm vectors must hold {c} elements, got {[v.numel() for v in vs]}')
    return fp(vs[0]), fp(vs[1]), fp(vs[2]), fp(vs[3]), float(eps)


def _nhwc_empty(b, c, h, w, device):
    return torch.empty((b, c, h, w), dtype=torch.float32, device=device, memory_format=torch.channels_last)


def bn_prelu(x, bn, slope, want_y=True, bn_next=None, sub_stride=0):
    """t = prelu(bn(x), slope) in one pass over x [B,C,H,W] (channels_last storage); bn = (mean, var, gamma, beta, eps) of
    an eval-mode BatchNorm2d.  Returns (y, y_next, y_sub): y = t when want_y, y_next = bn_next(t) when bn_next is given,
    y_sub = t[:, :, ::s, ::s] when sub_stride = s >= 1; the others are None.  None (alone) when the kernel does not
    serve the shape (C % 4 != 0): the caller then runs the modules."""
    b, c, h, w = _nhwc(x, 'bn_prelu input')
    if not (want_y or bn_next is not None or sub_stride >= 1):
        raise ValueError('bn_prelu: no output requested')
    slope = slope.contiguous()
    if slope.numel() != c:
        raise ValueError(f'bn_prelu: {slope.numel()} slopes for {c} channels')
    y = torch.empty_like(x) if want_y else None
    y_next = torch.empty_like(x) if bn_next is not None else None
    y_sub = None
    if sub_stride >= 1:
        y_sub = _nhwc_empty(b, c, (h - 1) // sub_stride + 1, (w - 1) // sub_stride + 1, x.device)
    with launching(x, 'bn_prelu', (b, c, h, w)) as stream:
        st = lib().fmgan_bn_prelu_f32(fp(x), *_bn_args(bn, c), fp(slope), fp(y), *_bn_args(bn_next, c), fp(y_next),
                                      fp(y_sub), b, c, h, w, max(int(sub_stride), 0), stream)
    return (y, y_next, y_sub) if served(st, 'bn_prelu') else None


def se_pool(r):
    """Per-(sample, channel) partial sums over row chunks of r [B,C,H,W] (channels_last storage) -> [B, chunks, C];
    fixed order, no atomics.  None when the kernel does not serve the shape."""
    b, c, h, w = _nhwc(r, 'se_pool input')
    chunks = lib().fmgan_se_pool_chunks(b, c, h, w)
    if chunks <= 0:
        return None
    partial = torch.empty((b, chunks, c), dtype=torch.float32, device=r.device)
    with launching(r, 'se_pool', (b, c, h, w)) as stream:
        st = lib().fmgan_se_pool_f32(fp(r), fp(partial), b, c, h, w, stream)
    return partial if served(st, 'se_pool') else None


def se_gate(partial, hw, bn, fc1, fc2):
    """gate [B,C] = sigmoid(fc2 . relu(fc1 . bn(sum_k partial[:, k] / hw))) from se_pool's partials [B, chunks, C]; fc1,
    fc2 the SE module's 1x1 convolution weights ([C/r, C, 1, 1] and [C, C/r, 1, 1], or 2-D).  None when not served."""
    require_gpu(partial, 'se_gate partials')
    b, chunks, c = partial.shape
    mid = fc1.shape[0]
    if tuple(fc1.shape[:2]) != (mid, c) or tuple(fc2.shape[:2]) != (c, mid) or fc1.numel() != mid * c \
            or fc2.numel() != mid * c:
        raise ValueError(f'se_gate: fc1 {tuple(fc1.shape)} / fc2 {tuple(fc2.shape)} do not fit {c} channels')
    fc1, fc2, partial = fc1.reshape(mid, c).contiguous(), fc2.reshape(c, mid).contiguous(), partial.contiguous()
    gate = torch.empty((b, c), dtype=torch.float32, device=partial.device)
    with launching(partial, 'se_gate', (b, c, mid, chunks)) as stream:
        st = lib().fmgan_se_gate_f32(fp(partial), chunks, int(hw), *_bn_args(bn, c), fp(fc1), fp(fc2), fp(gate), b, c,
                                     mid, stream)
    return gate if served(st, 'se_gate') else None


def ir_tail(r, bn, gate, shortcut, sc_stride=1, bn_sc=None, bn_next=None):
    """out = bn(r) * gate[b, c] + shortcut in one pass; r [B,C,H,W] (channels_last storage), gate [B,C] or None.
    bn_sc given: shortcut [B,C,H,W] is the 1x1 shortcut convolution's output and bn_sc is applied to it; otherwise it is
    the unit's input [B,C,Hs,Ws], read in place at every sc_stride-th pixel (MaxPool2d(1, sc_stride)).  Returns
    (out, out_next) with out_next = bn_next(out) or None; None (alone) when the kernel does not serve the shape."""
    b, c, h, w = _nhwc(r, 'ir_tail input')
    sb, scc, sh, sw = _nhwc(shortcut, 'ir_tail shortcut')
    exp = (h, w) if bn_sc is not None else ((sh - 1) // sc_stride + 1, (sw - 1) // sc_stride + 1)
    if (sb, scc) != (b, c) or exp != (h, w) or (bn_sc is not None and ((sh, sw) != (h, w) or sc_stride != 1)):
        raise ValueError(f'ir_tail: shortcut {tuple(shortcut.shape)} at stride {sc_stride} does not cover {tuple(r.shape)}')
    if gate is not None:
        if tuple(gate.shape) != (b, c):
            raise ValueError(f'ir_tail: gate {tuple(gate.shape)} for {tuple(r.shape)}')
        gate = gate.contiguous()
    out = torch.empty_like(r)
    out_next = torch.empty_like(r) if bn_next is not None else None
    with launching(r, 'ir_tail', (b, c, h, w, sc_stride, bn_sc is not None)) as stream:
        st = lib().fmgan_ir_tail_f32(fp(r), *_bn_args(bn, c), fp(gate), fp(shortcut), sh, sw, int(sc_stride),
                                     *_bn_args(bn_sc, c), fp(out), *_bn_args(bn_next, c), fp(out_next), b, c, h, w, stream)
    return (out, out_next) if served(st, 'ir_tail') else None


def modconv_demod(weight, style, scale, eps=1e-8, wsq=None):
    """weight [cout,cin,k,k] (or [1,cout,cin,k,k]) f32, style [B,cin] -> demod [B,cout].
    wsq: optional cached modconv_wsq(weight) — same bits, 1/k^2 of the reads."""
    cout, cin, kh, kw = weight.shape[-4:]
    style = style.contiguous()
    demod = torch.empty((style.shape[0], cout), dtype=torch.float32, device=style.device)
    with on_device(style) as stream:
        if wsq is not None:
            check(lib().fmgan_modconv_demod_wsq_f32(fp(wsq), fp(style), fp(demod), style.shape[0], cout, cin,
                                                    float(scale), float(eps), stream), 'modconv_demod_wsq')
        else:
            check(lib().fmgan_modconv_demod_f32(fp(weight), fp(style), fp(demod), style.shape[0], cout, cin,
                                                kh * kw, float(scale), float(eps), stream), 'modconv_demod')
    return demod


def equal_linear(x, weight, bias=None):
    """out = x @ weight.T (+ bias): x [B,K] f32, weight [N,K] f32 (already scaled), bias [N] or None -> [B,N]."""
    require_gpu(x, 'input')
    x, weight = x.contiguous(), weight.contiguous()
    b, k = x.shape
    n = weight.shape[0]
    if weight.shape[1] != k:
        raise RuntimeError(f'equal_linear: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}')
    out = torch.empty((b, n), dtype=torch.float32, device=x.device)
    with on_device(x) as stream:
        check(lib().fmgan_equal_linear_f32(fp(x), fp(weight), fp(bias), fp(out), b, n, k, stream), 'equal_linear')
    return out


def style_bank(table, n_entries, w, wplus, styles_out):
    """Every table entry's style in one launch (op/style_bank.py builds the table): w [T,D], wplus [P,n_styles,D] with
    P in {1, T}, styles_out flat f32 of T * sum(cin) elements."""
    if w.dim() != 2 or wplus.dim() != 3 or wplus.shape[2] != w.shape[1] or not (w.is_contiguous() and wplus.is_contiguous()):
        raise RuntimeError(f'style_bank: W {tuple(w.shape)} / W+ {tuple(wplus.shape)} must be contiguous [T,D] / [P,n,D]')
    with on_device(w) as stream:
        check(lib().fmgan_style_bank_f32(fp(table.view(torch.float32)), n_entries, fp(w), fp(wplus), wplus.shape[0],
                                         w.shape[0], w.shape[1], fp(styles_out), stream), 'style_bank')


def demod_bank(table, n_entries, styles, batch, demod_out):
    """Every demodulated table entry's coefficients in one launch, from the flat styles of style_bank()."""
    with on_device(styles) as stream:
        check(lib().fmgan_demod_bank_f32(fp(table.view(torch.float32)), n_entries, fp(styles), batch, fp(demod_out), stream),
              'demod_bank')


def modconv_wsq(weight):
    """[.., cout,cin,k,k] -> per-(o,i) sum of squared taps [cout,cin] (input of modconv_demod(wsq=...))."""
    cout, cin, kh, kw = weight.shape[-4:]
    wsq = torch.empty((cout, cin), dtype=torch.float32, device=weight.device)
    with on_device(weight) as stream:
        check(lib().fmgan_modconv_wsq_f32(fp(weight), fp(wsq), cout, cin, kh * kw, stream), 'modconv_wsq')
    return wsq


def modconv_weight_prep(weight, scale, kind=0):
    """[.., cout,cin,k,k] -> MFMA A-operand layout of scale*weight: kind 0 [cin, k*k, cout] (forward);
    kind 1 [cout, k*k, cin] with flipped taps (data-gradient of the plain conv); kind 2 [cout, k*k, cin]
    (data-gradient of the transposed conv)."""
    cout, cin, kh, kw = weight.shape[-4:]
    shape = (cin, kh * kw, cout) if kind == 0 else (cout, kh * kw, cin)
    wt = torch.empty(shape, dtype=torch.float32, device=weight.device)
    with on_device(weight) as stream:
        check(lib().fmgan_modconv_weight_prep_f32(fp(weight), fp(wt), cout, cin, kh * kw, float(scale), int(kind),
                                                  stream), 'modconv_weight_prep')
    return wt


def aligned_rows_shape(b, c, oh, ow, pad0):
    """(storage shape, element offset of logical (0,0,0,0), plane stride, row stride) of aligned_rows_buffer."""
    off = pad0 % 4
    rs = (ow + off + 31) // 32 * 32
    return (b * c, oh, rs), off, oh * rs, rs


def aligned_rows_buffer(b, c, oh, ow, pad0, device):
    """Private conv_transpose -> blur intermediate: rows padded to a multiple of 32 floats (one 128-byte line) and
    shifted right by pad0 (mod 4) floats, so that the blur's first tap column (x = -pad0) sits on a 16-byte boundary
    and every wave-wide 1 KiB row load covers exactly 8 cache lines.  Measured on the 1024^2 blur (MI355X):
    contiguous 2W+1 rows 512-527 us, 16-byte-aligned rows 498 us, line-aligned rows 438-450 us (= copy speed).
    Returns (storage, data_ptr of logical element (0,0,0,0), plane stride, row stride) — strides in elements."""
    shape, off, ps, rs = aligned_rows_shape(b, c, oh, ow, pad0)
    buf = torch.empty(shape, dtype=torch.float32, device=device)
    return buf, buf.data_ptr() + 4 * off, ps, rs


# Contraction of modconv2d: 'f32' (default, the parity path: v_mfma_f32_32x32x2_f32), 'bf16' (bf16 MFMA operands, fp32
# accumulation; BASELINE config 5's reduced-precision leg) or 'bf16x3' (fp32 operands split into three bf16 pieces, six
# bf16 MFMAs per product: fp32 accuracy at 2.7x the fp32 matrix rate; forward only, labelled).  Context manager only.
_mc_precision = 'f32'


class modconv_precision:
    """`with modconv_precision('bf16'):` — every modconv2d call inside (forward and data-gradient contractions of the
    modulated conv) whose shape the bf16 kernel serves runs on v_mfma_f32_32x32x16_bf16; the rest stay fp32."""

    def __init__(self, precision):
        if precision not in ('f32', 'bf16', 'bf16x3'):
            raise ValueError("precision must be 'f32', 'bf16' or 'bf16x3'")
        self.precision = precision

    def __enter__(self):
        global _mc_precision
        self.prev, _mc_precision = _mc_precision, self.precision
        return self

    def __exit__(self, *exc):
        global _mc_precision
        _mc_precision = self.prev
        return False


def modconv_weight_to_bf16(wt):
    """fp32 MFMA layout wt [cin, taps, cout] (modconv_weight_prep) -> bf16 operand image (opaque int16 tensor)."""
    cin, taps, cout = wt.shape
    nbytes = lib().fmgan_modconv_weight_bf16_bytes(cin, cout, taps)
    wtb = torch.empty(nbytes // 2, dtype=torch.int16, device=wt.device)
    with on_device(wt) as stream:
        check(lib().fmgan_modconv_weight_to_bf16(fp(wt), ptr(wtb), cin, cout, taps, stream), 'modconv_weight_to_bf16')
    return wtb


def wino_weight(wt):
    """fp32 MFMA layout wt [cin, 9, cout] (scaled) -> Winograd F(2x2,3x3) weight U [16, cout, cin]."""
    cin, taps, cout = wt.shape
    if taps != 9:
        raise RuntimeError('wino_weight: 3x3 weights only')
    u = torch.empty((16, cout, cin), dtype=torch.float32, device=wt.device)
    with on_device(wt) as stream:
        check(lib().fmgan_wino_weight_f32(fp(wt), fp(u), cin, cout, stream), 'wino_weight')
    return u


def wino_input(x, style):
    """The input transform alone: x [B,cin,H,W] (H, W even), style [B,cin] -> V [16, cin, B*(H/2)*(W/2)]."""
    require_gpu(x, 'input')
    x, style = x.contiguous(), style.contiguous()
    b, cin, h, w = x.shape
    v = torch.empty((16, cin, b * (h // 2) * (w // 2)), dtype=torch.float32, device=x.device)
    with on_device(x) as stream:
        check(lib().fmgan_wino_input_f32(fp(x), fp(style), fp(v), b, cin, h, w, stream), 'wino_input')
    return v


def wino_output(m, demod, batch, h, w, noise=None, noise_weight=None, bias=None, fuse_act=False, alpha=0.2,
                act_scale=2 ** 0.5):
    """The output transform + StyledConv epilogue alone: M [16, cout, B*(H/2)*(W/2)] -> out [B,cout,H,W]."""
    require_gpu(m, 'm')
    m = m.contiguous()
    cout = m.shape[1]
    if m.shape[0] != 16 or m.shape[2] != batch * (h // 2) * (w // 2):
        raise RuntimeError('wino_output: M must be [16, cout, B*(H/2)*(W/2)]')
    out = torch.empty((batch, cout, h, w), dtype=torch.float32, device=m.device)
    nz, nb = _noise_args(noise)
    with on_device(m) as stream:
        check(lib().fmgan_wino_output_f32(fp(m), fp(demod), fp(nz), fp(noise_weight), fp(bias), fp(out), batch, cout, h, w,
                                          nb, int(bool(fuse_act)), float(alpha), float(act_scale), stream), 'wino_output')
    return out


def modconv2d_winograd(x, wt, style, demod, noise=None, noise_weight=None, bias=None, fuse_act=False, alpha=0.2,
                       act_scale=2 ** 0.5, u=None):
    """Plain 3x3 modulated conv in Winograd F(2x2,3x3) form: input transform (own kernel), 16 batched fp32 GEMMs (torch.bmm ->
    the BLAS library), output transform + StyledConv epilogue (own kernel).  x [B,cin,H,W] with H, W even; wt as for
    modconv2d (or u = wino_weight(wt) prepared by the caller)."""
    require_gpu(x, 'input')
    x, style = x.contiguous(), style.contiguous()
    b, cin, h, w = x.shape
    if (h | w) & 1:
        raise RuntimeError('modconv2d_winograd: H and W must be even')
    if u is None:
        u = wino_weight(wt)
    cout = u.shape[1]
    n = b * (h // 2) * (w // 2)
    v = torch.empty((16, cin, n), dtype=torch.float32, device=x.device)
    m = torch.empty((16, cout, n), dtype=torch.float32, device=x.device)
    out = torch.empty((b, cout, h, w), dtype=torch.float32, device=x.device)
    nz, nb = _noise_args(noise)
    with launching(x, 'modconv2d_winograd', (b, cin, cout, h, w, 0)) as stream:      # one bracket round the three steps
        check(lib().fmgan_wino_input_f32(fp(x), fp(style), fp(v), b, cin, h, w, stream), 'wino_input')
        torch.bmm(u, v, out=m)
        st = lib().fmgan_wino_output_f32(fp(m), fp(demod), fp(nz), fp(noise_weight), fp(bias), fp(out), b, cout, h, w,
                                         nb, int(bool(fuse_act)), float(alpha), float(act_scale), stream)
    check(st, 'wino_output')
    return out


def modconv_weight_to_bf16x3(wt):
    """fp32 MFMA layout wt [cin, taps, cout] -> its three bf16 operand images (hi, mid, lo) in one opaque tensor."""
    cin, taps, cout = wt.shape
    nbytes = lib().fmgan_modconv_weight_bf16x3_bytes(cin, cout, taps)
    wts = torch.empty(nbytes // 2, dtype=torch.int16, device=wt.device)
    with on_device(wt) as stream:
        check(lib().fmgan_modconv_weight_to_bf16x3(fp(wt), ptr(wts), cin, cout, taps, stream), 'modconv_weight_to_bf16x3')
    return wts


def conv_weight_to_bf16x3(weight):
    """A Conv2d weight [cout, cin, 3, 3] (any memory format) -> the split-operand image of conv3x3s2_bf16x3: the
    [cin, 9, cout] order, then modconv_weight_to_bf16x3.  One bracket ('conv_weight_bf16x3') round the two steps."""
    require_gpu(weight, 'weight')
    cout, cin, kh, kw = weight.shape
    with launching(weight, 'conv_weight_bf16x3', (cout, cin, kh * kw)):
        wt = weight.detach().permute(1, 2, 3, 0).reshape(cin, kh * kw, cout).contiguous()
        return modconv_weight_to_bf16x3(wt)


def conv3x3s2_bf16x3_supported(batch, cin, cout, h, w):
    return bool(lib().fmgan_conv3x3s2_bf16x3_supported(int(batch), int(cin), int(cout), int(h), int(w)))


def conv3x3s2_bf16x3(x, wts, bias, cout, alpha=0.01, channels_last=False):
    """LeakyReLU(conv3x3(x, stride 2, pad 1) + bias) with fp32 operands split into three bf16 pieces (fp32 accumulation).
    x [B,cin,H,W] f32 NCHW-contiguous, wts = conv_weight_to_bf16x3(weight), bias [cout] or None.  Returns
    [B,cout,(H-1)//2+1,(W-1)//2+1] — NCHW-contiguous, or in channels_last storage (written so by the kernel: what the
    MIOpen tail of a style head reads) — or None where the library declines the shape."""
    require_gpu(x, 'input')
    if not x.is_contiguous():
        raise RuntimeError(f'conv3x3s2_bf16x3: input must be NCHW-contiguous, got strides {x.stride()}')
    b, cin, h, w = x.shape
    out = torch.empty((b, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=x.device,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    with launching(x, 'conv3x3s2_bf16x3', (b, cin, cout, h, w)) as stream:
        st = lib().fmgan_conv3x3s2_bf16x3_f32(fp(x), ptr(wts), fp(bias), fp(out), b, cin, cout, h, w, float(alpha),
                                              int(bool(channels_last)), stream)
    return out if served(st, 'conv3x3s2_bf16x3') else None


def current_modconv_precision():
    return _mc_precision


def modconv2d(x, wt, style, demod, mode, noise=None, noise_weight=None, bias=None, fuse_act=False, alpha=0.2,
              act_scale=2 ** 0.5, strided_out=None, precision=None):
    """x [B,cin,H,W] f32, wt from modconv_weight_prep (3x3), style [B,cin], demod [B,cout] or None.
    strided_out = (ptr, plane_stride, row_stride) writes into a caller-owned strided buffer and returns None.
    precision: None = the ambient modconv_precision (default 'f32')."""
    require_gpu(x, 'input')
    x = x.contiguous()
    style = style.contiguous()
    b, cin, h, w = x.shape
    cout = wt.shape[2]
    oh, ow = (2 * h + 1, 2 * w + 1) if mode == 1 else (((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == 2 else (h, w))
    if strided_out is None:
        out = torch.empty((b, cout, oh, ow), dtype=torch.float32, device=x.device)
        out_ptr, ops, ors = out.data_ptr(), 0, 0
    else:
        out = None
        out_ptr, ops, ors = strided_out
    nz, nb = _noise_args(noise)
    prec, L = precision or _mc_precision, lib()
    # one launch for the three contractions: the name (also the observer's), the per-call weight image, the extra arguments
    if prec == 'bf16x3' and L.fmgan_modconv2d_bf16x3_supported(b, cin, cout, h, w, mode):
        name, wtb, extra = 'modconv2d_bf16x3', modconv_weight_to_bf16x3(wt), ()
    elif prec == 'bf16' and L.fmgan_modconv2d_bf16_supported(b, cin, cout, h, w, mode):
        name, wtb, extra = 'modconv2d_bf16', modconv_weight_to_bf16(wt), ()
    else:
        ws_bytes = L.fmgan_modconv2d_workspace_bytes(b, cin, cout, h, w, mode)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device) if ws_bytes else None
        name, wtb, extra = 'modconv2d', None, (fp(ws), ws_bytes)
    launch = getattr(L, 'fmgan_' + name + ('_f32' if wtb is None else ''))
    with launching(x, name, (b, cin, cout, h, w, mode)) as stream:
        st = launch(fp(x), fp(wt) if wtb is None else ptr(wtb), fp(style), fp(demod), out_ptr, b, cin, cout, h, w, mode,
                    fp(nz), fp(noise_weight), fp(bias), nb, int(bool(fuse_act)), float(alpha), float(act_scale), ops, ors,
                    *extra, stream)
    check(st, name)
    return out


def modconv2d_rgb_fusable(batch, cin, cout, h, w):
    return bool(lib().fmgan_modconv2d_rgb_fusable(int(batch), int(cin), int(cout), int(h), int(w)))


def modconv2d_select(batch, cin, cout, h, w, mode, rgb=False, has_workspace=True):
    """(cfg, variant letter, BM, BN, ksplit): the tile and split-K factor modconv2d (rgb: modconv2d_rgb) launches for this
    shape — host logic, no device needed.  Raises as the launch would for arguments it refuses."""
    v = [ctypes.c_int() for _ in range(5)]
    check(lib().fmgan_modconv2d_select(int(batch), int(cin), int(cout), int(h), int(w), int(mode), int(bool(rgb)),
                                       int(bool(has_workspace)), *[ctypes.byref(c) for c in v]), 'modconv2d_select')
    cfg, variant, bm, bn, ks = (c.value for c in v)
    return cfg, chr(variant) if variant else '', bm, bn, ks


def modconv2d_tiles():
    """Tiles of this build of the library: [(mode, cfg, variant letter, BM, BN, fuses_rgb), ...] in table order."""
    n = lib().fmgan_modconv2d_tiles(None, 0)
    buf = (ctypes.c_int * (6 * n))()
    lib().fmgan_modconv2d_tiles(buf, n)
    return [(buf[6 * k], buf[6 * k + 1], chr(buf[6 * k + 2]), buf[6 * k + 3], buf[6 * k + 4], bool(buf[6 * k + 5]))
            for k in range(n)]


def modconv2d_rgb(x, wt, style, demod, noise, noise_weight, bias, alpha, act_scale, rgb_weight, rgb_style, rgb_bias,
                  rgb_skip, rgb_scale, keep_out=True):
    """Plain 3x3 modulated conv + noise/bias/LeakyReLU with the following ToRGB (1x1 modulated conv + bias + skip) in
    the same kernel.  Returns (activation or None, rgb [B,3,H,W]).  Shapes must satisfy modconv2d_rgb_fusable()."""
    require_gpu(x, 'input')
    x = x.contiguous()
    style, rgb_style = style.contiguous(), rgb_style.contiguous()
    b, cin, h, w = x.shape
    cout = wt.shape[2]
    rgb_c = rgb_weight.numel() // cout
    out = torch.empty((b, cout, h, w), dtype=torch.float32, device=x.device) if keep_out else None
    rgb = torch.empty((b, rgb_c, h, w), dtype=torch.float32, device=x.device)
    nz, nb = _noise_args(noise)
    sk = rgb_skip.contiguous() if rgb_skip is not None else None
    wmod = torch.empty((b, 3, cout), dtype=torch.float32, device=x.device)
    with on_device(x) as stream:                                  # the per-forward ToRGB weight: outside the bracket
        check(lib().fmgan_torgb_weight_mod_f32(fp(rgb_weight), fp(rgb_style), fp(wmod), b, cout, rgb_c,
                                               float(rgb_scale), stream), 'torgb_weight_mod')
    with launching(x, 'modconv2d', (b, cin, cout, h, w, 0)) as stream:
        st = lib().fmgan_modconv2d_rgb_f32(fp(x), fp(wt), fp(style), fp(demod), fp(out), b, cin, cout, h, w,
                                           fp(nz), fp(noise_weight), fp(bias), nb, 1, float(alpha), float(act_scale),
                                           fp(wmod), fp(rgb_bias), fp(sk), fp(rgb), rgb_c, stream)
    check(st, 'modconv2d_rgb')
    return out, rgb


def modconv_wgrad(go, demod, x, style, scale, fast_only=False, mode=0):
    """Conv part of the weight gradient of the modulated conv (mode as in modconv2d; x is the conv's input, go the
    gradient of its output) -> [cout,cin,3,3]; None if the shape is not served by the kernel, or — with fast_only — not
    by its 64 x 64-tile form (>= 48 channels on both sides)."""
    go, x, style = go.contiguous(), x.contiguous(), style.contiguous()
    b, cout = go.shape[:2]
    cin, h, w = x.shape[1:]
    if (fast_only or mode != 0) and (cin < 48 or cout < 48):
        return None
    ws_bytes = lib().fmgan_modconv_wgrad_mode_workspace_bytes(b, cin, cout, h, w, int(mode))
    if ws_bytes == 0:
        return None
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device)
    with launching(x, 'modconv_wgrad', (b, cin, cout, h, w, int(mode))) as stream:
        st = lib().fmgan_modconv_wgrad_mode_f32(fp(go), fp(demod), fp(x), fp(style), fp(gw), b, cin, cout, h, w,
                                                int(mode), float(scale), fp(ws), ws_bytes, stream)
    check(st, 'modconv_wgrad')
    return gw


def torgb(x, weight, style, bias, skip, scale):
    """x [B,cin,H,W] f32, weight [cout,cin] (any leading/trailing 1 dims), style [B,cin], bias [cout], skip [B,cout,H,W]."""
    require_gpu(x, 'input')
    x = x.contiguous()
    style = style.contiguous()
    b, cin, h, w = x.shape
    cout = weight.numel() // cin
    sk = skip.contiguous() if skip is not None else None
    out = torch.empty((b, cout, h, w), dtype=torch.float32, device=x.device)
    with launching(x, 'torgb', (b, cin, cout, h * w)) as stream:
        st = lib().fmgan_torgb_f32(fp(x), fp(weight), fp(style), fp(bias), fp(sk), fp(out), b, cin, cout, h * w,
                                   float(scale), stream)
    check(st, 'torgb')
    return out


def torgb_backward(x, grad_out, weight, style, scale):
    """Data gradient of ToRGB's 1x1 modulated conv and the pixel contraction M[b,c,i] = sum_p grad_out[b,c,p]*x[b,i,p]
    from one pass over x.  Returns (grad_x [B,cin,H,W], M [B,cout,cin]) or None when the kernel does not serve the
    shape (H*W % 4 != 0, not f32)."""
    require_gpu(x, 'input')
    if x.dtype != torch.float32 or grad_out.dtype != torch.float32:
        return None
    x, go, style = x.contiguous(), grad_out.contiguous(), style.contiguous()
    b, cin, h, w = x.shape
    cout = weight.numel() // cin
    splits = lib().fmgan_torgb_backward_splits(b, cin, h * w)
    if splits == 0 or cout > 4:
        return None
    gx = torch.empty_like(x)
    mpart = torch.empty((splits, b, cout, cin), dtype=torch.float32, device=x.device)
    wgt = weight.contiguous()
    with launching(x, 'torgb_backward', (b, cin, cout, h * w)) as stream:
        st = lib().fmgan_torgb_backward_f32(fp(x), fp(go), fp(wgt), fp(style), fp(gx), fp(mpart), b, cin, cout, h * w,
                                            float(scale), stream)
    if not served(st, 'torgb_backward'):
        return None
    return gx, (mpart.sum(0) if splits > 1 else mpart[0])


def images_to_tensor(images, mean=0.5, std=0.5):
    """uint8 [B,H,W,3] (GPU) -> float32 [B,3,H,W] = ((images/255) - mean)/std: ToTensor + Normalize in one pass."""
    require_gpu(images, 'images')
    if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[-1] != 3:
        raise RuntimeError('images_to_tensor: expected a uint8 [B,H,W,3] tensor')
    x = images.contiguous()
    b, h, w, _ = x.shape
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=x.device)
    with on_device(x) as stream:
        check(lib().fmgan_images_to_tensor(ptr(x), ptr(out), b, h, w, float(mean), float(std), stream), 'images_to_tensor')
    return out


def resize_output_size(h, w, size):
    """torchvision Resize(int) rule: (out_h, out_w) for an [h, w] image (host logic, no GPU needed)."""
    oh, ow = ctypes.c_int(), ctypes.c_int()
    check(lib().fmgan_resize_output_size(int(h), int(w), int(size), ctypes.byref(oh), ctypes.byref(ow)), 'resize_output_size')
    return oh.value, ow.value


def resize_plan(in_h, in_w, out_h, out_w):
    """Pillow's bilinear coefficient tables for this size pair as a CPU int32 tensor (host logic, no GPU needed)."""
    n = lib().fmgan_resize_plan_ints(int(in_h), int(in_w), int(out_h), int(out_w))
    if n <= 0:
        raise RuntimeError('resize_plan: invalid sizes')
    plan = torch.empty(n, dtype=torch.int32)
    check(lib().fmgan_resize_plan(int(in_h), int(in_w), int(out_h), int(out_w), plan.data_ptr(), n), 'resize_plan')
    return plan


_PLANS = {}


def resize_images(images, out_h, out_w, to_tensor=False, mean=0.5, std=0.5):
    """uint8 [B,H,W,3] (GPU) -> PIL-exact bilinear resize.  to_tensor=False: uint8 [B,out_h,out_w,3];
    to_tensor=True: float32 [B,3,out_h,out_w] = ((v/255) - mean)/std (Resize + ToTensor + Normalize in one pass)."""
    require_gpu(images, 'images')
    if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[-1] != 3:
        raise RuntimeError('resize_images: expected a uint8 [B,H,W,3] tensor')
    x = images.contiguous()
    b, h, w, _ = x.shape
    key = (x.device, h, w, out_h, out_w)
    plan = _PLANS.get(key)
    if plan is None:
        plan = _PLANS[key] = resize_plan(h, w, out_h, out_w).to(x.device)
    if to_tensor:
        out = torch.empty((b, 3, out_h, out_w), dtype=torch.float32, device=x.device)
        o8, o32 = None, out
    else:
        out = torch.empty((b, out_h, out_w, 3), dtype=torch.uint8, device=x.device)
        o8, o32 = out, None
    with launching(x, 'resize', (b, h, w, out_h, out_w)) as stream:
        st = lib().fmgan_resize_bilinear_u8(ptr(x), ptr(plan), ptr(o8), ptr(o32), b, h, w, out_h, out_w, float(mean),
                                            float(std), stream)
    check(st, 'resize_bilinear_u8')
    return out


def tensor_to_images(tensor, cent=1.0, factor=255.0 / 2.0):
    """float32 [B,3,H,W] (GPU) -> uint8 [B,H,W,3] = uint8((clip(t,-1,1)+cent)*factor): tensor2im for the whole batch."""
    require_gpu(tensor, 'tensor')
    if tensor.dtype != torch.float32 or tensor.ndim != 4 or tensor.shape[1] != 3:
        raise RuntimeError('tensor_to_images: expected a float32 [B,3,H,W] tensor')
    x = tensor.contiguous()
    b, _, h, w = x.shape
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=x.device)
    with on_device(x) as stream:
        check(lib().fmgan_tensor_to_images(ptr(x), ptr(out), b, h, w, float(cent), float(factor), stream), 'tensor_to_images')
    return out


def tiles_to_canvas(src, canvas, slots, tile, cent=1.0, factor=255.0 / 2.0):
    """float32 [n,3,s,s] tiles into square slots of the uint8 canvas batch [C,H,W,3], in place, one launch
    (csrc/image_io.hip): slots int32 [n,3] ON src's DEVICE, one (canvas, y0, x0) per tile; s = tile, 2*tile or 4*tile (the
    tile is reduced by aten's bilinear rule).  The raw entry: op/canvas.py checks the layout on the host beforehand; the
    kernel skips a slot that does not lie inside its canvas.  Tensors of another dtype, device or layout are refused."""
    if src.ndim != 4 or src.shape[1] != 3 or src.shape[2] != src.shape[3] or canvas.ndim != 4 or canvas.shape[3] != 3 \
            or slots.ndim != 2 or tuple(slots.shape) != (src.shape[0], 3):
        raise ValueError(f'tiles_to_canvas: src {tuple(src.shape)}, canvas {tuple(canvas.shape)}, slots '
                         f'{tuple(slots.shape)}: expected [n, 3, s, s], [C, H, W, 3] and [n, 3]')
    require_f32_gpu('tiles_to_canvas', ((src, 'src'),))
    for t, name, dtype in ((canvas, 'canvas', torch.uint8), (slots, 'slots', torch.int32)):
        require_gpu(t, name)
        if t.dtype != dtype or not t.is_contiguous() or t.device != src.device:
            raise RuntimeError(f'tiles_to_canvas: {name} must be a contiguous {dtype} tensor on src\'s device, got '
                               f'{t.dtype} on {t.device} with strides {t.stride()}')
    n, _, s, _ = src.shape
    nc, ch, cw, _ = canvas.shape
    if n == 0:
        return canvas
    with launching(src, 'tiles_to_canvas', (n, s, int(tile), nc, ch, cw)) as stream:
        st = lib().fmgan_tiles_to_canvas(fp(src), ptr(canvas), ctypes.cast(slots.data_ptr(), ctypes.POINTER(ctypes.c_int)),
                                         n, s, int(tile), nc, ch, cw, float(cent), float(factor), stream)
    check(st, 'tiles_to_canvas')
    return canvas


BANK_GATHER_BANKS, BANK_GATHER_GROUPS = 4, 8      # csrc/image_bank.hip: BG_MAX_BANKS, BG_MAX_GROUPS


def bank_gather(banks, index_a, index_b, offset, members, stride, groups, mean=0.5, std=0.5, out=None,
                pixels_per_lane=0):
    """out[s] = ((bank[k_s][i_s] / 255) - mean) / std in one launch (csrc/image_bank.hip): `banks` up to 4 uint8
    [N_k,H,W,3] GPU tensors of one H x W (contiguous; a view into a larger storage is fine), index_a / index_b int32 GPU
    tensors (index_b may be None), `groups` a sequence of (bank, source, swap, mul, add); returns float32
    [len(groups) * members, 3, H, W], group after group.  The raw entry: op/image_bank.py checks index ranges and the
    pairing on the host beforehand; the kernel skips a slot whose bank, position or image index is out of range.
    Tensors of another dtype, device or layout are refused.  members == 0: an empty tensor, no launch."""
    banks = list(banks)
    groups = [tuple(int(v) for v in g) for g in groups]
    if not 1 <= len(banks) <= BANK_GATHER_BANKS or not 1 <= len(groups) <= BANK_GATHER_GROUPS \
            or any(len(g) != 5 for g in groups):
        raise ValueError(f'bank_gather: {len(banks)} banks and {len(groups)} groups: 1..{BANK_GATHER_BANKS} banks and '
                         f'1..{BANK_GATHER_GROUPS} groups of (bank, source, swap, mul, add)')
    first = banks[0]
    for k, t in enumerate(banks):
        require_gpu(t, f'banks[{k}]')
        if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[3] != 3 or not t.is_contiguous() or t.device != first.device:
            raise RuntimeError(f'bank_gather: banks[{k}] must be a contiguous uint8 [N,H,W,3] tensor on banks[0]\'s '
                               f'device, got {t.dtype} {tuple(t.shape)} on {t.device} with strides {t.stride()}')
        if tuple(t.shape[1:3]) != tuple(first.shape[1:3]):
            raise ValueError(f'bank_gather: banks[{k}] holds {tuple(t.shape[1:3])} images, banks[0] '
                             f'{tuple(first.shape[1:3])}')
    for t, name in ((index_a, 'index_a'), (index_b, 'index_b')):
        if t is None and name == 'index_b':
            continue
        require_gpu(t, name)
        if t.dtype != torch.int32 or t.ndim != 1 or not t.is_contiguous() or t.device != first.device:
            raise RuntimeError(f'bank_gather: {name} must be a contiguous int32 vector on the banks\' device')
    h, w = int(first.shape[1]), int(first.shape[2])
    members, n = int(members), int(members) * len(groups)
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=first.device)
    else:
        require_f32_gpu('bank_gather', ((out, 'out'),))
        if tuple(out.shape) != (n, 3, h, w) or out.device != first.device:
            raise ValueError(f'bank_gather: out {tuple(out.shape)} on {out.device}, expected {(n, 3, h, w)} on '
                             f'{first.device}')
    if n == 0:
        return out
    ptrs = [ptr(t) for t in banks] + [None] * (BANK_GATHER_BANKS - len(banks))
    counts = [int(t.shape[0]) for t in banks] + [0] * (BANK_GATHER_BANKS - len(banks))
    table = (ctypes.c_int * (5 * len(groups)))(*[v for g in groups for v in g])
    with launching(first, 'bank_gather', (n, h, w, len(groups), int(stride))) as stream:
        st = lib().fmgan_bank_gather(*ptrs, *counts, h, w, ptr(index_a), int(index_a.numel()), ptr(index_b),
                                     0 if index_b is None else int(index_b.numel()), int(offset), members, int(stride),
                                     table, len(groups), fp(out), float(mean), float(std), int(pixels_per_lane), stream)
    check(st, 'bank_gather')
    return out


# ----------------------------------------------------------------------------- L-BFGS (csrc/lbfgs.hip)
# The five launches of a fused FullBatchLBFGS step over the buffers of an op.lbfgs.FusedState `s` (it has made the device,
# dtype and layout checks); `table`: the ctypes segment table of lbfgs_segments.
def lbfgs_segments(params):
    """(table, nseg) for the entry points: 3 long long per parameter, {parameter address, gradient address or 0, numel}."""
    vals = []
    for p in params:
        vals += [p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr(), p.numel()]
    return (ctypes.c_longlong * len(vals))(*vals), len(vals) // 3


def lbfgs_pair(s, table, nseg, t, has_pair):
    with launching(s.g, 'lbfgs_pair', (s.n, s.m, bool(has_pair))) as stream:
        st = lib().fmgan_lbfgs_pair_f32(ctypes.addressof(table), nseg, fp(s.g), fp(s.g_prev), fp(s.d), fp(s.S), fp(s.Y),
                                        s.state.data_ptr(), s.partial.data_ptr(), s.n, s.m, float(t), int(has_pair),
                                        stream)
    check(st, 'lbfgs_pair')


def lbfgs_coeffs(s, t, eps, has_pair):
    with launching(s.g, 'lbfgs_coeffs', (s.n, s.m, bool(has_pair))) as stream:
        st = lib().fmgan_lbfgs_coeffs_f64(s.partial.data_ptr(), s.G.data_ptr(), s.state.data_ptr(), s.record.data_ptr(),
                                          s.coef.data_ptr(), s.n, s.m, float(t), float(eps), int(has_pair), stream)
    check(st, 'lbfgs_coeffs')


def lbfgs_direction(s):
    with launching(s.g, 'lbfgs_direction', (s.n, s.m)) as stream:
        st = lib().fmgan_lbfgs_direction_f32(s.coef.data_ptr(), s.state.data_ptr(), fp(s.S), fp(s.Y), fp(s.g),
                                             fp(s.g_prev), fp(s.d), s.partial.data_ptr(), s.record.data_ptr(), s.n, s.m,
                                             stream)
    check(st, 'lbfgs_direction')


def lbfgs_update(s, table, nseg, a):
    with launching(s.g, 'lbfgs_update', (s.n,)) as stream:
        st = lib().fmgan_lbfgs_update_f32(ctypes.addressof(table), nseg, fp(s.d), float(a), s.n, stream)
    check(st, 'lbfgs_update')


def lbfgs_gather(s, table, nseg):
    with launching(s.g, 'lbfgs_gather', (s.n,)) as stream:
        st = lib().fmgan_lbfgs_gather_f32(ctypes.addressof(table), nseg, fp(s.g_new), fp(s.d), s.partial.data_ptr(),
                                          s.record.data_ptr(), s.n, stream)
    check(st, 'lbfgs_gather')


# ----------------------------------------------------------------------------- training loop (csrc/train_loop.hip)
EMA_CHUNK = 4096                          # elements per block of fmgan_ema_f32 (csrc/train_loop.hip EMA_CHUNK)
LOSS_ROW_COLUMNS = 16                     # pointers of fmgan_loss_ptrs, columns of a ledger row


def ema_blocks(numel):
    return int(lib().fmgan_ema_blocks(int(numel)))


def ema(table, n_entries, total_blocks, decay, numel=0):
    """dst <- decay * dst + (1 - decay) * src over every entry of `table` (a uint8 GPU tensor holding n_entries
    fmgan_ema_entry, built by op.ema.EmaPlan, which has made the device, dtype, layout and overlap checks) in one launch
    on the current stream of the table's device.  decay travels as float(decay) and float(1 - decay), the difference
    taken in double."""
    require_gpu(table, 'table')
    decay = float(decay)
    with launching(table, 'ema', (int(n_entries), int(total_blocks), int(numel))) as stream:
        st = lib().fmgan_ema_f32(table.data_ptr(), int(n_entries), int(total_blocks), ctypes.c_float(decay),
                                 ctypes.c_float(1.0 - decay), stream)
    check(st, 'ema')


def loss_row(values, row):
    """One row of the loss log in one launch: values, at most 16 entries, each None or a one-element float32 tensor on
    row's device; row, a contiguous float32 GPU vector of 16 elements (a row of the ledger's ring).  row[i] = values[i]
    (0.0 for None and for the columns past len(values))."""
    n = len(values)
    if n > LOSS_ROW_COLUMNS:
        check(FMGAN_EINVAL, f'loss_row: {n} values for {LOSS_ROW_COLUMNS} columns')
    require_f32_gpu('loss_row', ((row, 'row'),))
    if row.numel() != LOSS_ROW_COLUMNS:
        raise ValueError(f'loss_row: row of {row.numel()} elements, expected {LOSS_ROW_COLUMNS}')
    ptrs = (ctypes.c_void_p * LOSS_ROW_COLUMNS)()
    for k, v in enumerate(values):
        if v is None:
            continue
        if v.numel() != 1 or v.device != row.device:
            raise RuntimeError(f'loss_row: value {k} must hold one element on {row.device}, got {tuple(v.shape)} on '
                               f'{v.device}')
        ptrs[k] = fp(v)
    with launching(row, 'loss_row', (n,)) as stream:
        st = lib().fmgan_loss_row_f32(ctypes.addressof(ptrs), n, fp(row), stream)
    check(st, 'loss_row')
