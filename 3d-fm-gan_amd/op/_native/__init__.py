"""ctypes binding of libfmgan_hip.so (include/fmgan_hip.h) — the only way the host code reaches a kernel.

There is NO fallback: if the library is missing, or a tensor is not on the GPU, this raises.
PyTorch is used for device memory and streams only; every launch goes on torch's current HIP stream
of the tensor's device (as the reference launches on at::cuda::getCurrentCUDAStream,
op/upfirdn2d_kernel.cu:213-215), asynchronously, so calls can be captured in a HIP graph.

core.py holds the library, its signature table, the checks and the launch bracket; a wrapper lives in the module of the
csrc file that defines its entry point.  Callers use `_native.<name>`: every public name is re-exported here.  Mutable
state (core._lib, core._observer, activation._act_io, conv._mc_precision) has one owner and is read there at call time.
"""
from .core import (  # noqa: F401
    LIB_PATH, F32, F64, F16, BF16, FMGAN_OK, FMGAN_EINVAL, FMGAN_EUNSUPPORTED, amp_fwd, amp_bwd, lib, check, served,
    require_gpu, dtype_code, ptr, fp, require_f32_gpu, on_device, nhwc_dense, set_observer, launching)
from .activation import (  # noqa: F401
    activation_io, current_activation_io, io16, amp_fwd_io, BLUR_PATHS, upfirdn2d_out_size, upfirdn2d,
    upfirdn2d_strided, blur_noise_bias_act_serves, blur_noise_bias_act, fused_bias_act, fused_bias_act_backward,
    noise_bias_act, prelu_backward, dtype16_code, upfirdn2d16, fused_bias_act16, fused_bias_act16_backward)
from .conv import (  # noqa: F401
    modconv_demod, modconv_wsq, modconv_weight_prep, aligned_rows_shape, aligned_rows_buffer, modconv_precision,
    current_modconv_precision, modconv2d, modconv2d_rgb_fusable, modconv2d_select, modconv2d_tiles, modconv2d_rgb,
    modconv_weight_to_bf16, modconv_weight_to_bf16x3, conv_weight_to_bf16x3, conv3x3s2_bf16x3_supported,
    conv3x3s2_bf16x3, conv3x3_bf16x3_supported, conv3x3_bf16x3, C3_EPILOGUES, conv3x3_tail_bf16x3_select,
    conv3x3_tail_bf16x3, modconv_wgrad, modconv_wgrad_select, wino_select, wino_weight,
    wino_input, wino_output, modconv2d_winograd, torgb,
    torgb_backward, equal_linear, style_bank, style_bank_concat, demod_bank)
from .encoder import bn_prelu, se_pool, se_gate, ir_tail  # noqa: F401
from .loss import (  # noqa: F401
    LPIPS_SIZE, face_region_loss, face_region_loss_backward, render_mask, lpips_distance, lpips_distance_backward,
    lpips_pair_input, projection_loss_fwd, projection_loss_bwd, HEATMAP_SIZE, face_crop_serves, face_crop_fwd,
    face_crop_bwd, detector_input, heatmap_distance_serves, heatmap_distance_fwd, heatmap_distance_bwd,
    landmark_decode)
from .evaluation import (  # noqa: F401
    face_input_pool, face_input, f64p, fid_stats_serves, fid_stats_update, fid_stats_finish, INCEPTION_SIZE,
    inception_input)
from .image import (  # noqa: F401
    images_to_tensor, resize_output_size, resize_plan, resize_images, tensor_to_images, tiles_to_canvas,
    BANK_GATHER_BANKS, BANK_GATHER_GROUPS, bank_gather)
from .optim import (  # noqa: F401
    lbfgs_segments, lbfgs_pair, lbfgs_coeffs, lbfgs_direction, lbfgs_update, lbfgs_gather, EMA_CHUNK,
    LOSS_ROW_COLUMNS, ema_blocks, ema, loss_row)
