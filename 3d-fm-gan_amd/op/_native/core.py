"""The library itself: where libfmgan_hip.so is, its signature table (include/fmgan_hip.h), status codes, the pointer and
device checks every wrapper makes, and the launch bracket with its observer.  No wrapper of a kernel lives here."""
import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))        # the directory that holds op/
LIB_PATH = os.environ.get('FMGAN_LIB') or os.path.join(_PKG, 'csrc', 'libfmgan_hip.so')

F32, F64, F16 = 0, 1, 2
BF16 = 3                                  # the 16-bit activation kernels only (csrc/act16.hip)
FMGAN_OK, FMGAN_EINVAL, FMGAN_EUNSUPPORTED = 0, -1, -2      # include/fmgan_hip.h, status codes
_DTYPES = {torch.float32: F32, torch.float64: F64, torch.float16: F16}

_lib = None

# Under torch.autocast (BASELINE config 5's bf16 leg) the MIOpen convolutions hand bf16 tensors to their consumers; the
# HIP kernels compute in fp32 (their reference counterparts dispatch float / double / half only): every custom autograd
# Function of this package is entered with autocast off and its floating-point CUDA inputs cast to fp32.  A no-op when
# autocast is not active.
amp_fwd = torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
amp_bwd = torch.amp.custom_bwd(device_type='cuda')


class ambient:
    """An ambient switch as a context manager: `with switch(value):` validates the value, stores it in the owning module's
    variable and puts the previous one back on leaving, also when the body raises.  A subclass names its `values`, the
    ValueError `text`, and its variable as (`scope`, `var`): the owning module's globals() and the variable's name, so
    that the module's functions read the plain global at call time."""
    values, text, scope, var = (), '', None, ''

    def __init__(self, value):
        if value not in self.values:
            raise ValueError(self.text)
        self.value = value

    def __enter__(self):
        self.prev, self.scope[self.var] = self.scope[self.var], self.value
        return self

    def __exit__(self, *exc):
        self.scope[self.var] = self.prev
        return False


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
    # csrc/abi.hip
    _sig(L.fmgan_abi_version, [])
    _sig(L.fmgan_status_string, [i], ctypes.c_char_p)
    _sig(L.fmgan_refresh_entry_bytes, [])
    # csrc/upfirdn2d.hip
    _sig(L.fmgan_upfirdn2d_select, [i] * 15)
    _sig(L.fmgan_upfirdn2d_out_size, [i] * 12 + [ctypes.POINTER(i)] * 2)
    _sig(L.fmgan_upfirdn2d, [i, vp, vp, vp] + [i] * 15 + [vp])
    _sig(L.fmgan_upfirdn2d_strided, [i, vp, vp, vp] + [i] * 4 + [ll, i] + [i] * 11 + [vp])
    _sig(L.fmgan_blur_noise_bias_act_f32, [vp] * 3 + [i] * 4 + [ll, i] + [i] * 6 + [vp] * 3 + [i, f, f, vp])
    _sig(L.fmgan_blur_noise_bias_act_select, [vp] * 3 + [i] * 4 + [ll, i] + [i] * 6)
    _sig(L.fmgan_blur_noise_bias_act_path_f32, [vp] * 3 + [i] * 4 + [ll, i] + [i] * 6 + [vp] * 3 + [i, f, f, i, vp])
    # csrc/fused_bias_act.hip
    _sig(L.fmgan_fused_bias_act, [i, vp, vp, vp, vp, ll, i, i, i, i, f, f, vp])
    _sig(L.fmgan_noise_bias_act_f32, [vp] * 5 + [i] * 4 + [f, f, vp])
    _sig(L.fmgan_fused_bias_act_bwd_blocks, [ll, i])
    _sig(L.fmgan_fused_bias_act_bwd_f32, [vp] * 4 + [ll, i, f, f, vp])
    _sig(L.fmgan_prelu_backward_blocks, [ll, i])
    _sig(L.fmgan_prelu_backward_f32, [vp] * 5 + [ll, i, vp])
    # csrc/act16.hip
    _sig(L.fmgan_act16_fba_select, [i, ll, i, i, i, i])
    _sig(L.fmgan_act16_fba, [i, vp, vp, vp, vp, ll, i, i, i, i, f, f, vp])
    _sig(L.fmgan_act16_fba_bwd_blocks, [ll, i])
    _sig(L.fmgan_act16_fba_bwd, [i] + [vp] * 4 + [ll, i, f, f, vp])
    _sig(L.fmgan_ufd16_select, [i] * 15)
    _sig(L.fmgan_ufd16, [i, vp, vp, vp] + [i] * 14 + [vp])
    # csrc/modconv_prep.hip
    _sig(L.fmgan_modconv_demod_f32, [vp] * 3 + [i] * 4 + [f, f, vp])
    _sig(L.fmgan_modconv_wsq_f32, [vp] * 2 + [i] * 3 + [vp])
    _sig(L.fmgan_modconv_demod_wsq_f32, [vp] * 3 + [i] * 3 + [f, f, vp])
    _sig(L.fmgan_modconv_weight_prep_f32, [vp, vp, i, i, i, f, i, vp])
    # csrc/modconv_fwd.hip
    _sig(L.fmgan_modconv2d_workspace_bytes, [i] * 6, ll)
    _sig(L.fmgan_modconv2d_f32, [vp] * 5 + [i] * 6 + [vp] * 3 + [i, i, f, f, ll, i, vp, ll, vp])
    _sig(L.fmgan_modconv2d_rgb_fusable, [i] * 5)
    _sig(L.fmgan_modconv2d_select, [i] * 8 + [ctypes.POINTER(i)] * 5)
    _sig(L.fmgan_modconv2d_tiles, [ctypes.POINTER(i), i])
    _sig(L.fmgan_modconv2d_rgb_f32, [vp] * 5 + [i] * 5 + [vp] * 3 + [i, i, f, f] + [vp] * 4 + [i, vp])
    # csrc/modconv_bf16.hip
    _sig(L.fmgan_modconv_weight_bf16_bytes, [i] * 3, ll)
    _sig(L.fmgan_modconv_weight_to_bf16, [vp, vp, i, i, i, vp])
    _sig(L.fmgan_modconv2d_bf16_supported, [i] * 6)
    _sig(L.fmgan_modconv2d_bf16, [vp] * 5 + [i] * 6 + [vp] * 3 + [i, i, f, f, ll, i, vp])
    _sig(L.fmgan_modconv_weight_bf16x3_bytes, [i] * 3, ll)
    _sig(L.fmgan_modconv_weight_to_bf16x3, [vp, vp, i, i, i, vp])
    _sig(L.fmgan_modconv2d_bf16x3_supported, [i] * 6)
    _sig(L.fmgan_modconv2d_bf16x3, [vp] * 5 + [i] * 6 + [vp] * 3 + [i, i, f, f, ll, i, vp])
    # csrc/conv3x3_x3.hip
    _sig(L.fmgan_conv3x3s2_bf16x3_supported, [i] * 5)
    _sig(L.fmgan_conv3x3s2_bf16x3_f32, [vp] * 4 + [i] * 5 + [f, i, vp])
    _sig(L.fmgan_conv3x3_bf16x3_supported, [i] * 7)
    _sig(L.fmgan_conv3x3_bf16x3_f32, [vp] * 4 + [i] * 9 + [f, vp])
    _sig(L.fmgan_conv3x3_tail_bf16x3_select, [i] * 5)
    _sig(L.fmgan_conv3x3_tail_bf16x3_f32, [vp] * 4 + [i] * 5 + [f, i, vp])
    # csrc/modconv_wgrad.hip
    _sig(L.fmgan_modconv_wgrad_workspace_bytes, [i] * 5, ll)
    _sig(L.fmgan_modconv_wgrad_f32, [vp] * 5 + [i] * 5 + [f, vp, ll, vp])
    _sig(L.fmgan_modconv_wgrad_mode_workspace_bytes, [i] * 6, ll)
    _sig(L.fmgan_modconv_wgrad_mode_f32, [vp] * 5 + [i] * 6 + [f, vp, ll, vp])
    _sig(L.fmgan_modconv_wgrad_select, [i] * 7 + [ctypes.POINTER(i)] * 7)
    # csrc/winograd.hip
    _sig(L.fmgan_wino_select, [i] * 6)
    _sig(L.fmgan_wino_weight_f32, [vp, vp, i, i, vp])
    _sig(L.fmgan_wino_input_f32, [vp] * 3 + [i] * 4 + [vp])
    _sig(L.fmgan_wino_output_f32, [vp] * 6 + [i] * 6 + [f, f, vp])
    # csrc/torgb.hip
    _sig(L.fmgan_torgb_weight_mod_f32, [vp] * 3 + [i] * 3 + [f, vp])
    _sig(L.fmgan_torgb_f32, [vp] * 6 + [i] * 4 + [f, vp])
    _sig(L.fmgan_torgb_backward_splits, [i] * 3)
    _sig(L.fmgan_torgb_backward_f32, [vp] * 6 + [i] * 4 + [f, vp])
    # csrc/linear.hip
    _sig(L.fmgan_equal_linear_f32, [vp] * 4 + [i] * 3 + [vp])
    # csrc/style_bank.hip
    _sig(L.fmgan_style_bank_entry_bytes, [])
    _sig(L.fmgan_style_bank_f32, [vp, i, vp, vp, i, i, i, vp, vp])
    _sig(L.fmgan_style_bank_concat_f32, [vp, i, vp, vp, i, i, i, i, vp, vp])
    _sig(L.fmgan_demod_bank_f32, [vp, i, vp, i, vp, vp])
    # csrc/live_weights.hip
    _sig(L.fmgan_weight_refresh_blocks, [i, i, i, i, ll], ll)
    _sig(L.fmgan_weight_refresh_f32, [vp, i, ll, vp])
    # csrc/encoder_glue.hip
    _sig(L.fmgan_bn_prelu_f32, [vp] * 5 + [f, vp, vp] + [vp] * 4 + [f, vp, vp] + [i] * 5 + [vp])
    _sig(L.fmgan_se_pool_chunks, [i] * 4)
    _sig(L.fmgan_se_pool_f32, [vp, vp] + [i] * 4 + [vp])
    _sig(L.fmgan_se_gate_f32, [vp, i, ll] + [vp] * 4 + [f] + [vp] * 3 + [i] * 3 + [vp])
    _sig(L.fmgan_ir_tail_f32, [vp] * 5 + [f, vp, vp] + [i] * 3 + [vp] * 4 + [f, vp] + [vp] * 4 + [f, vp] + [i] * 4 + [vp])
    # csrc/face_region.hip
    _sig(L.fmgan_face_region_blocks, [i, ll])
    _sig(L.fmgan_face_region_loss_f32, [vp] * 3 + [i, i, ll, vp])
    _sig(L.fmgan_face_region_backward_f32, [vp] * 4 + [i, i, ll, vp])
    _sig(L.fmgan_render_mask_f32, [vp] * 2 + [i, i, ll, vp])
    # csrc/lpips_distance.hip
    _sig(L.fmgan_lpips_distance_blocks, [i] * 3)
    _sig(L.fmgan_lpips_distance_f32, [vp] * 4 + [i, i, i, f, vp])
    _sig(L.fmgan_lpips_distance_backward_f32, [vp] * 6 + [i, i, i, f, vp])
    # csrc/ppl_input.hip
    _sig(L.fmgan_lpips_pair_input_select, [i] * 8)
    _sig(L.fmgan_lpips_pair_input_f32, [vp] * 5 + [i] * 8 + [vp])
    # csrc/projection_loss.hip
    _sig(L.fmgan_projection_loss_select, [i] * 4)
    _sig(L.fmgan_projection_loss_blocks, [i] * 4)
    _sig(L.fmgan_projection_loss_fwd_f32, [vp] * 7 + [i] * 4 + [vp])
    _sig(L.fmgan_projection_loss_bwd_f32, [vp] * 7 + [i] * 4 + [vp])
    # csrc/landmark.hip
    _sig(L.fmgan_face_crop_select, [i] * 4)
    _sig(L.fmgan_face_crop_fwd_f32, [vp] * 3 + [i] * 4 + [vp])
    _sig(L.fmgan_face_crop_bwd_f32, [vp] * 3 + [i] * 4 + [vp])
    _sig(L.fmgan_detector_input_f32, [vp, vp, i, ll, vp])
    _sig(L.fmgan_heatmap_distance_blocks, [i, ll])
    _sig(L.fmgan_heatmap_distance_fwd_f32, [vp] * 3 + [i, ll, vp])
    _sig(L.fmgan_heatmap_distance_bwd_f32, [vp] * 5 + [i, ll, vp])
    _sig(L.fmgan_landmark_decode_f32, [vp] * 5 + [i] * 4 + [vp])
    # csrc/eval_scores.hip
    _sig(L.fmgan_face_input_blocks, [i] * 4)
    _sig(L.fmgan_face_input_f32, [vp] * 5 + [i] * 4 + [vp])
    # csrc/fid_stats.hip
    _sig(L.fmgan_fid_stats_select, [i] * 2)
    _sig(L.fmgan_fid_stats_update_f32, [vp] * 4 + [i, i, vp])
    _sig(L.fmgan_fid_stats_finish_f64, [vp] * 3 + [ll, vp, vp, i, vp])
    # csrc/inception_input.hip
    _sig(L.fmgan_inception_input_select, [i] * 3)
    _sig(L.fmgan_inception_input_f32, [vp, vp] + [i] * 4 + [vp])
    # csrc/image_io.hip
    _sig(L.fmgan_images_to_tensor, [vp, vp, i, i, i, f, f, vp])
    _sig(L.fmgan_resize_bilinear_u8, [vp] * 4 + [i] * 5 + [f, f, vp])
    _sig(L.fmgan_tensor_to_images, [vp, vp, i, i, i, f, f, vp])
    _sig(L.fmgan_tiles_to_canvas, [vp, vp, ctypes.POINTER(i)] + [i] * 6 + [f, f, vp])
    # csrc/resize_plan.cpp
    _sig(L.fmgan_resize_output_size, [i, i, i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)])
    _sig(L.fmgan_resize_plan_ints, [i] * 4, ll)
    _sig(L.fmgan_resize_plan, [i] * 4 + [vp, ll])
    # csrc/image_bank.hip
    _sig(L.fmgan_bank_gather, [vp] * 4 + [i] * 6 + [vp, ll, vp, ll, ll, i, i, ctypes.POINTER(i), i, vp, f, f, i, vp])
    # csrc/lbfgs.hip
    _sig(L.fmgan_lbfgs_pair_blocks, [ll], ll)
    _sig(L.fmgan_lbfgs_pair_f32, [vp, i] + [vp] * 7 + [ll, i, f, i, vp])
    _sig(L.fmgan_lbfgs_coeffs_f64, [vp] * 5 + [ll, i, f, f, i, vp])
    _sig(L.fmgan_lbfgs_direction_f32, [vp] * 9 + [ll, i, vp])
    _sig(L.fmgan_lbfgs_update_f32, [vp, i, vp, f, ll, vp])
    _sig(L.fmgan_lbfgs_gather_f32, [vp, i] + [vp] * 4 + [ll, vp])
    # csrc/train_loop.hip
    _sig(L.fmgan_ema_blocks, [ll], ll)
    _sig(L.fmgan_ema_f32, [vp, i, ll, f, f, vp])
    _sig(L.fmgan_loss_row_f32, [vp, i, vp, vp])
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


def nhwc_dense(t):
    """Is the [N, C, H, W] tensor stored as one dense [N, H, W, C] block (channels_last with nothing between pixels)?"""
    return t.ndim == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def _nhwc_empty(b, c, h, w, device):
    return torch.empty((b, c, h, w), dtype=torch.float32, device=device, memory_format=torch.channels_last)


# ----------------------------------------------------------------------------- launch observer (bench.py)
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
