"""Composition of the hot path: (photo, render) -> image  (reference: Util/network_util.py).

Kept for the callers (train_3_encoder.py:460,507,574; Evaluation/visual_eval.py:116,180,296; quant_eval.py:93,162):
Forward_Inference_3_Encoder, Forward_Inference (the 2-encoder scheme: plain and the three co-modulation modes),
Build_Generator_From_Dict, Get_Network_Shape, Get_Conv_Kernel_Key.
Re-animation (one photo, a sequence of renders: the reference's GIF driver, Evaluation/visual_eval.py:147-186, which
re-runs all three encoders per frame): Encode_Photo once, then Forward_Inference_Reanimate / Reanimate_From_Codes per
chunk of frames; for the 2-encoder scheme Encode_Photo_2_Encoder, then Forward_Inference_Reanimate_2_Encoder /
Reanimate_From_Codes_2_Encoder.
Image/PIL helpers of the reference file (torchvision-based) are not on the path and not provided.
"""
import os
from typing import NamedTuple, Optional

import torch

from op import _native
from op.style_bank import comod_column, concat_column, sliced_columns
from stylegan2 import Generator
from Util.streams import side_streams, run_on, overlap_ok

MODULATION_ENCODING = ['Render Image', 'Photo Image']
CO_MODULATION_MODE = ['Multiplication', 'Concatenation', 'Tensor Transform']


def Get_Conv_Kernel_Key(model_dict):
    """Keys of the main-path modulated conv weights, first to last (Util/network_util.py:22-36)."""
    return ['conv1.conv.weight'] + [k for k in model_dict.keys() if 'convs' in k and 'conv.weight' in k]


def Get_Network_Shape(model_dict):
    """Channel widths per synthesis layer, inferred from the conv weight shapes [1,Cout,Cin,k,k] (:39-50)."""
    keys = Get_Conv_Kernel_Key(model_dict)
    return [model_dict[k].shape[2] for k in keys] + [model_dict[keys[-1]].shape[1]]


def Build_Generator_From_Dict(model_dict, size=256, latent=512, n_mlp=8):
    """Generator whose (possibly pruned) widths are read off a state_dict, then loaded (:101-115)."""
    generator = Generator(size, latent, n_mlp, generator_net_shape=Get_Network_Shape(model_dict))
    generator.load_state_dict(model_dict, strict=False)
    return generator


def _unwrapped(net):
    # The reference reads g_ema.module.n_latent and therefore only works on a DataParallel-wrapped generator
    # (Util/network_util.py:317-318).  DDP and Miscellaneous.distributed.Replica also expose .module;
    # a bare Generator is accepted too.
    return getattr(net, 'module', net)


PIPELINE = os.environ.get('FMGAN_NO_PIPELINE', '0') != '1'
# Side streams share the device's 4 hardware queues with the main stream: measured on MI355X (pairs1024), ResNets on
# one stream + 2 head streams 339.8 pairs/s; 2 + 2: 335; 2 + 4: 325; 8 hardware queues (GPU_MAX_HW_QUEUES): 246.
RESNET_STREAMS = int(os.environ.get('FMGAN_RESNET_STREAMS', '1'))


def _pipelined(p_input, r_input, tsr_input, E_Tsr, E_W, e_wp, g_ema, sliced_layer, use_tanh):
    """Inference schedule of Forward_Inference_3_Encoder: the synthesis network consumes W+ one column per layer, so it
    starts as soon as the first style heads of the pSp encoder are done and runs beside the remaining heads (each a
    large conv followed by a tail of tiny launches) instead of after all of them.  Same arithmetic per element as the
    serial form: latent[:, i] = W * W+[:, i] (or W), image = g(latent, tsr)."""
    rs = side_streams(p_input.device, RESNET_STREAMS, 'resnets')
    s1, s2 = rs[0], rs[-1]
    join1, encoded_tensor = run_on(s1, E_Tsr, tsr_input)
    join2, encoded_W = run_on(s2, E_W, r_input)
    heads = e_wp.forward_deferred(p_input)
    join1(); join2()
    sliced = sliced_columns(sliced_layer, _unwrapped(g_ema).n_latent, len(heads))
    cache = {}

    def column(i):
        if i not in cache:
            wait, wp = heads[i]
            wait()
            cache[i] = comod_column(encoded_W, wp, i, sliced)
        return cache[i]

    g_output = g_ema(noise_z=None, use_external_input_tensor=True, external_input_tensor=encoded_tensor,
                     latent_columns=column)
    for wait, _ in heads:          # columns the generator did not read: still join their streams
        wait()
    return torch.tanh(g_output) if use_tanh else g_output


def Forward_Inference_3_Encoder(p_input, r_input, E_Tsr, E_W, E_W_Plus, g_ema, tsr_encode='Photo Image',
                                sliced_layer=None, use_tanh=False, PPL_regularize=False):
    """One forward of the 3-encoder scheme with multiplicative co-modulation (Util/network_util.py:293-338).

    tsr = E_Tsr(photo | render) [N,512,4,4];  W = E_W(render) [N,512];  W+ = E_W_Plus(photo) [N,n_latent,512];
    latent[:, i] = W * W+[:, i] for i in sliced_layer else W;  image = g_ema(latent, external_input_tensor=tsr).
    """
    if tsr_encode not in MODULATION_ENCODING:
        raise ValueError(f'tsr_encode must be one of {MODULATION_ENCODING}')
    tsr_input = p_input if tsr_encode == 'Photo Image' else r_input
    if (PIPELINE and overlap_ok(p_input) and not PPL_regularize and hasattr(_unwrapped(E_W_Plus), 'forward_deferred')
            and isinstance(_unwrapped(g_ema), Generator)):
        return _pipelined(p_input, r_input, tsr_input, E_Tsr, E_W, _unwrapped(E_W_Plus), g_ema, sliced_layer, use_tanh)
    if overlap_ok(p_input):
        # the three encoders are independent: the two small ResNets run on side streams beside the pSp encoder
        rs = side_streams(p_input.device, RESNET_STREAMS, 'resnets')
        join1, encoded_tensor = run_on(rs[0], E_Tsr, tsr_input)
        join2, encoded_W = run_on(rs[-1], E_W, r_input)
        encoded_W_plus = E_W_Plus(p_input)
        join1(); join2()
    else:
        encoded_tensor = E_Tsr(tsr_input)
        encoded_W = E_W(r_input)
        encoded_W_plus = E_W_Plus(p_input)

    n_styles = encoded_W_plus.shape[1]
    sliced = sliced_columns(sliced_layer, _unwrapped(g_ema).n_latent, n_styles)
    # W (.) W+ where sliced, W elsewhere.  Built from device tensors only (no host-side mask upload), so the whole
    # forward stays capturable in a HIP graph.
    if len(sliced) == n_styles:
        encoded_latent = encoded_W.unsqueeze(1) * encoded_W_plus
    else:
        encoded_latent = torch.stack([comod_column(encoded_W, encoded_W_plus[:, i], i, sliced) for i in range(n_styles)], 1)

    g_output = g_ema(noise_z=None, latent_styles=[encoded_latent], input_is_latent=True,
                     use_external_input_tensor=True, external_input_tensor=encoded_tensor,
                     PPL_regularize=PPL_regularize)
    if use_tanh:
        if PPL_regularize:
            g_output = (torch.tanh(g_output[0]),) + tuple(g_output[1:])
        else:
            g_output = torch.tanh(g_output)
    return g_output


class PhotoCode(NamedTuple):
    """What the photo contributes to every frame: W+ [P,n_styles,512] and, for tsr_encode='Photo Image', the 4x4 input
    tensor [P,512,4,4] (None for 'Render Image': the tensor then comes from each render)."""
    w_plus: torch.Tensor
    tensor: Optional[torch.Tensor]


def Encode_Photo(p_input, E_Tsr, E_W_Plus, tsr_encode='Photo Image'):
    """The photo side of Forward_Inference_3_Encoder, once: E_W_Plus (106 GFLOP per image) and, for 'Photo Image',
    E_Tsr on the ResNet side stream beside it.  Inference only (no_grad)."""
    if tsr_encode not in MODULATION_ENCODING:
        raise ValueError(f'tsr_encode must be one of {MODULATION_ENCODING}')
    _native.require_gpu(p_input, 'p_input')
    with torch.no_grad():
        if tsr_encode != 'Photo Image':
            return PhotoCode(E_W_Plus(p_input), None)
        if overlap_ok(p_input):
            join, tensor = run_on(side_streams(p_input.device, RESNET_STREAMS, 'resnets')[0], E_Tsr, p_input)
            w_plus = E_W_Plus(p_input)
            join()
        else:
            tensor, w_plus = E_Tsr(p_input), E_W_Plus(p_input)
    return PhotoCode(w_plus, tensor)


def Reanimate_From_Codes(photo_code, encoded_W, encoded_tensor, g_ema, sliced_layer=None, use_tanh=False, noise=None,
                         randomize_noise=True):
    """Frames [T,3,S,S] from stored codes: W [T,512] of the renders, the photo's PhotoCode (P = 1: shared by all
    frames, or P = T) and the input tensor [T,512,4,4] (None: the photo's, expanded over the frames).  Element for
    element the arithmetic of Forward_Inference_3_Encoder after its encoders: latent[:, i] = W * W+[:, i] where sliced,
    W elsewhere; image = g_ema(latent, tensor).  The generator is called bare (wrappers' `.module`), with the noise
    arguments given here."""
    frames = encoded_W.shape[0]
    tensor = photo_code.tensor if encoded_tensor is None else encoded_tensor
    if tensor is None:
        raise ValueError('no input tensor: the photo was encoded for \'Render Image\' and no encoded_tensor was given')
    if tensor.shape[0] != frames:
        if tensor.shape[0] != 1:
            raise ValueError(f'input tensor of {tensor.shape[0]} samples for {frames} frames')
        tensor = tensor.expand(frames, -1, -1, -1)
    with torch.no_grad():
        g_output = _unwrapped(g_ema)(noise_z=None, use_external_input_tensor=True,
                                     external_input_tensor=tensor.contiguous(), noise=noise,
                                     randomize_noise=randomize_noise,
                                     comod=(encoded_W, photo_code.w_plus, sliced_layer))
        return torch.tanh(g_output) if use_tanh else g_output


def Forward_Inference_Reanimate(photo_code, r_input, E_Tsr, E_W, g_ema, tsr_encode='Photo Image', sliced_layer=None,
                                use_tanh=False, noise=None, randomize_noise=True):
    """Render frames [T,3,256,256] + the photo's code -> images [T,3,S,S]: Forward_Inference_3_Encoder with the photo
    repeated T times, minus the photo-side encoders (40-55 % of a frame's arithmetic)."""
    if tsr_encode not in MODULATION_ENCODING:
        raise ValueError(f'tsr_encode must be one of {MODULATION_ENCODING}')
    _native.require_gpu(r_input, 'r_input')
    render_tsr = tsr_encode != 'Photo Image'
    with torch.no_grad():
        if overlap_ok(r_input):
            rs = side_streams(r_input.device, RESNET_STREAMS, 'resnets')
            join_t, encoded_tensor = run_on(rs[0], E_Tsr, r_input) if render_tsr else ((lambda: None), None)
            join_w, encoded_W = run_on(rs[-1], E_W, r_input)
            join_t(); join_w()
        else:
            encoded_tensor = E_Tsr(r_input) if render_tsr else None
            encoded_W = E_W(r_input)
    return Reanimate_From_Codes(photo_code, encoded_W, encoded_tensor, g_ema, sliced_layer, use_tanh, noise,
                                randomize_noise)


# ----------------------------------------------------------------------------------------------- the 2-encoder scheme
def _check_modes(mod_encode, co_modulation):
    if mod_encode not in MODULATION_ENCODING:
        raise ValueError(f'mod_encode must be one of {MODULATION_ENCODING}')
    if co_modulation is not None and co_modulation not in CO_MODULATION_MODE:
        raise ValueError(f'co_modulation must be None or one of {CO_MODULATION_MODE}')


def _encoder_inputs(p_input, r_input, mod_encode, co_modulation):
    """(input of the tensor encoder, input of the modulation encoder), Util/network_util.py:232-276: the plain mode
    follows mod_encode; every co-modulation mode encodes the render with the tensor encoder and the photo with the other."""
    if co_modulation is None and mod_encode == 'Render Image':
        return p_input, r_input
    return r_input, p_input


def _latent_2_encoder(co_modulation, encoded, encoded_W, sliced_layer, n_latent):
    """(latent for latent_styles, external input tensor or None) from the two encoders' outputs, element for element the
    reference's arithmetic: plain: (W or W+, tensor); 'Multiplication': columns V * W+[:, i] where sliced, V elsewhere;
    'Concatenation': [V | W+[:, i]]; 'Tensor Transform': the same with (tensor, V) from the tensor encoder."""
    if co_modulation is None:
        return encoded_W, encoded
    n_styles = encoded_W.shape[1]
    if co_modulation == 'Multiplication':
        sliced = sliced_columns(sliced_layer, n_latent, n_styles)
        return torch.stack([comod_column(encoded, encoded_W[:, i], i, sliced) for i in range(n_styles)], 1), None
    tensor, vec = encoded if co_modulation == 'Tensor Transform' else (None, encoded)
    return torch.cat([vec.unsqueeze(1).repeat(1, n_styles, 1), encoded_W], dim=2), tensor


def _tanh_image(g_output, PPL_regularize):
    """tanh on the image only; with PPL_regularize the output is (image, path_lengths): a new tuple."""
    if PPL_regularize:
        return (torch.tanh(g_output[0]),) + tuple(g_output[1:])
    return torch.tanh(g_output)


def _pipelined_2_encoder(tsr_input, mod_input, tensor_encoder, e_mod, g_ema, co_modulation, sliced_layer, use_tanh):
    """Inference schedule of Forward_Inference where the modulation encoder hands its W+ over one head at a time: the
    tensor encoder on a ResNet side stream, the synthesis network started on the first finished heads (latent_columns),
    each column composed as the serial form composes it.  A mode without an input tensor gets the Generator's own
    ConstantInput, repeated as the Generator would."""
    g = _unwrapped(g_ema)
    join, encoded = run_on(side_streams(tsr_input.device, RESNET_STREAMS, 'resnets')[0], tensor_encoder, tsr_input)
    heads = e_mod.forward_deferred(mod_input)
    join()
    if co_modulation is None:
        tensor, vec = encoded, None
    elif co_modulation == 'Tensor Transform':
        tensor, vec = encoded
    else:
        tensor, vec = g.input(encoded), encoded
    sliced = sliced_columns(sliced_layer, g.n_latent, len(heads))
    cache = {}

    def column(i):
        if i not in cache:
            wait, wp = heads[i]
            wait()
            if co_modulation is None:
                cache[i] = wp
            elif co_modulation == 'Multiplication':
                cache[i] = comod_column(vec, wp, i, sliced)
            else:
                cache[i] = concat_column(vec, wp)
        return cache[i]

    g_output = g_ema(noise_z=None, use_external_input_tensor=True, external_input_tensor=tensor, latent_columns=column)
    for wait, _ in heads:          # columns the generator did not read: still join their streams
        wait()
    return torch.tanh(g_output) if use_tanh else g_output


def Forward_Inference(p_input, r_input, tensor_encoder, modulation_encoder, g_ema, mod_encode='Render Image',
                      co_modulation=None, sliced_layer=None, use_tanh=False, PPL_regularize=False):
    """One forward of the 2-encoder scheme (Util/network_util.py:212-290).

    co_modulation None:  tensor = tensor_encoder(photo | render), W or W+ = modulation_encoder(render | photo) by
    mod_encode; image = g_ema(W or W+, external_input_tensor=tensor).
    'Multiplication':    V = tensor_encoder(render) [N,512], W+ = modulation_encoder(photo); latent[:, i] = V * W+[:, i]
    for i in sliced_layer else V; image = g_ema(latent) on the Generator's constant input.
    'Concatenation':     latent[:, i] = [V | W+[:, i]] ([N,n,1024]); image = g_ema(latent).
    'Tensor Transform':  (tensor, V) = tensor_encoder(render); the same latent; image = g_ema(latent, tensor).
    Under autograd this is the plain composite over the modules; in inference on the GPU the two encoders run on separate
    streams and, where the modulation encoder has forward_deferred, the synthesis network starts on its first heads."""
    _check_modes(mod_encode, co_modulation)
    tsr_input, mod_input = _encoder_inputs(p_input, r_input, mod_encode, co_modulation)
    if (PIPELINE and overlap_ok(p_input) and not PPL_regularize and hasattr(_unwrapped(modulation_encoder), 'forward_deferred')
            and isinstance(_unwrapped(g_ema), Generator)):
        return _pipelined_2_encoder(tsr_input, mod_input, tensor_encoder, _unwrapped(modulation_encoder), g_ema,
                                    co_modulation, sliced_layer, use_tanh)
    if overlap_ok(p_input):
        join, encoded = run_on(side_streams(p_input.device, RESNET_STREAMS, 'resnets')[0], tensor_encoder, tsr_input)
        encoded_W = modulation_encoder(mod_input)
        join()
    else:
        encoded = tensor_encoder(tsr_input)
        encoded_W = modulation_encoder(mod_input)
    latent, tensor = _latent_2_encoder(co_modulation, encoded, encoded_W, sliced_layer, _unwrapped(g_ema).n_latent)
    if tensor is None:
        g_output = g_ema(noise_z=None, latent_styles=[latent], input_is_latent=True, PPL_regularize=PPL_regularize)
    else:
        g_output = g_ema(noise_z=None, latent_styles=[latent], input_is_latent=True, use_external_input_tensor=True,
                         external_input_tensor=tensor, PPL_regularize=PPL_regularize)
    return _tanh_image(g_output, PPL_regularize) if use_tanh else g_output


class PhotoCode2(NamedTuple):
    """What the photo contributes to every frame in the 2-encoder scheme: `latent`, the modulation encoder's output
    (W+ [P,n_styles,512] in the co-modulation modes; W [P,512] or W+ in the plain mode with 'Photo Image'), or `tensor`,
    the 4x4 input tensor [P,512,4,4] (plain mode with 'Render Image').  The other one is None."""
    latent: Optional[torch.Tensor]
    tensor: Optional[torch.Tensor]


def Encode_Photo_2_Encoder(p_input, tensor_encoder, modulation_encoder, mod_encode='Render Image', co_modulation=None):
    """The photo side of Forward_Inference, once.  Inference only (no_grad)."""
    _check_modes(mod_encode, co_modulation)
    _native.require_gpu(p_input, 'p_input')
    with torch.no_grad():
        if co_modulation is None and mod_encode == 'Render Image':
            return PhotoCode2(None, tensor_encoder(p_input))
        return PhotoCode2(modulation_encoder(p_input), None)


def _over_frames(t, frames, what):
    if t.shape[0] == frames:
        return t
    if t.shape[0] != 1:
        raise ValueError(f'{what} of {t.shape[0]} samples for {frames} frames')
    return t.expand(frames, *t.shape[1:])


def Reanimate_From_Codes_2_Encoder(photo_code, frame_code, g_ema, mod_encode='Render Image', co_modulation=None,
                                   sliced_layer=None, use_tanh=False, noise=None, randomize_noise=True):
    """Frames [T,3,S,S] from stored codes: the photo's PhotoCode2 (P = 1: shared by all frames, or P = T) and what the
    per-frame encoder gave for the T renders — V [T,512] ('Multiplication', 'Concatenation'), (tensor [T,512,4,4],
    V [T,512]) ('Tensor Transform'), W [T,512] (plain, 'Render Image') or the tensor [T,512,4,4] (plain, 'Photo Image').
    Element for element the arithmetic of Forward_Inference after its encoders; the Generator is called bare, through
    comod= ('Multiplication'), comod_concat= (the concatenating modes) or the ordinary latent path (plain)."""
    _check_modes(mod_encode, co_modulation)
    g = _unwrapped(g_ema)
    kw = dict(noise_z=None, noise=noise, randomize_noise=randomize_noise)
    with torch.no_grad():
        if co_modulation is None:
            if mod_encode == 'Render Image':
                latent, tensor = frame_code, _over_frames(photo_code.tensor, frame_code.shape[0], 'input tensor')
            else:
                latent, tensor = _over_frames(photo_code.latent, frame_code.shape[0], 'latent'), frame_code
            g_output = g(latent_styles=[latent.contiguous()], input_is_latent=True, use_external_input_tensor=True,
                         external_input_tensor=tensor.contiguous(), **kw)
        elif co_modulation == 'Multiplication':
            g_output = g(comod=(frame_code, photo_code.latent, sliced_layer), **kw)
        elif co_modulation == 'Concatenation':
            g_output = g(comod_concat=(frame_code, photo_code.latent), **kw)
        else:
            tensor, vec = frame_code
            g_output = g(use_external_input_tensor=True, external_input_tensor=tensor.contiguous(),
                         comod_concat=(vec, photo_code.latent), **kw)
        return torch.tanh(g_output) if use_tanh else g_output


def Forward_Inference_Reanimate_2_Encoder(photo_code, r_input, tensor_encoder, modulation_encoder, g_ema,
                                          mod_encode='Render Image', co_modulation=None, sliced_layer=None, use_tanh=False,
                                          noise=None, randomize_noise=True):
    """Render frames [T,3,256,256] + the photo's code -> images [T,3,S,S]: Forward_Inference with the photo repeated T
    times, minus the photo-side encoder (in the co-modulation modes the pSp encoder, most of a frame's arithmetic)."""
    _check_modes(mod_encode, co_modulation)
    _native.require_gpu(r_input, 'r_input')
    per_frame = modulation_encoder if co_modulation is None and mod_encode == 'Render Image' else tensor_encoder
    with torch.no_grad():
        frame_code = per_frame(r_input)
    return Reanimate_From_Codes_2_Encoder(photo_code, frame_code, g_ema, mod_encode, co_modulation, sliced_layer,
                                          use_tanh, noise, randomize_noise)
