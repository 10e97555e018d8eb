"""StyleGAN2 Generator / Discriminator of 3D-FM GAN on MI355X kernels.

Same public API, constructor arguments, attribute names and state_dict keys as the reference's stylegan2.py
(so train_3_encoder.py / Evaluation/visual_eval.py / reference checkpoints work unchanged — pinned by
tests/golden/*_manifest.json), but the hot ops are hand-written gfx950 kernels reached through `op`:
  upfirdn2d, fused_leaky_relu           -> op.upfirdn2d / op.fused_act          (reference: op/*.cu)
  ModulatedConv2d 3x3 / transposed 3x3  -> op.modconv (MFMA implicit GEMM)      (reference: stylegan2.py:250-298)
  StyledConv epilogue (noise+bias+act)  -> fused into the conv epilogue when no graph is needed
  ToRGB (1x1 + bias + skip add)         -> one HBM pass                         (reference: stylegan2.py:389-404)
Host code stays PyTorch-ROCm.  There is no CPU path: CPU tensors raise RuntimeError in `op`.
"""
import math
import os
import random

import torch
from torch import nn, autograd
from torch.nn import functional as F

from op import FusedLeakyReLU, fused_leaky_relu, upfirdn2d
from op import _native, conv_grad, modconv, placement
from op._native import amp_fwd as _amp_fwd, amp_bwd as _amp_bwd
from op.live_weights import LiveWeights, live, live_u
from op.style_bank import Modulation, StyleBank, comod_column, concat_column, sliced_columns
from Util.streams import side_streams, run_on, overlap_ok

_SQRT2 = math.sqrt(2.0)


def _channel_table(channel_multiplier):
    # stylegan2.py:441-451 / 779-789
    table = {4: 512, 8: 512, 16: 512, 32: 512}
    for res, base in ((64, 256), (128, 128), (256, 64), (512, 32), (1024, 16)):
        table[res] = base * channel_multiplier
    return table


def make_kernel(k):
    """Normalised 2-D FIR from 1-D (outer product) or 2-D taps (stylegan2.py:36-44)."""
    k = torch.as_tensor(k, dtype=torch.float32)
    if k.ndim == 1:
        k = torch.outer(k, k)
    return k / k.sum()


class PixelNorm(nn.Module):
    """x / sqrt(mean_c(x^2) + 1e-8) (stylegan2.py:23-33)."""

    def forward(self, input):
        return input * torch.rsqrt(input.square().mean(dim=1, keepdim=True) + 1e-8)


class Upsample(nn.Module):
    """x`factor` FIR upsampling, taps * factor^2 (stylegan2.py:47-65)."""

    def __init__(self, kernel, factor=2):
        super().__init__()
        self.factor = factor
        self.register_buffer('kernel', make_kernel(kernel) * (factor ** 2))
        p = self.kernel.shape[0] - factor
        self.pad = ((p + 1) // 2 + factor - 1, p // 2)

    def forward(self, input):
        return upfirdn2d(input, self.kernel, up=self.factor, down=1, pad=self.pad)


class Downsample(nn.Module):
    """FIR decimation (stylegan2.py:68-86); defined for API parity, unused on the generator path."""

    def __init__(self, kernel, factor=2):
        super().__init__()
        self.factor = factor
        self.register_buffer('kernel', make_kernel(kernel))
        p = self.kernel.shape[0] - factor
        self.pad = ((p + 1) // 2, p // 2)

    def forward(self, input):
        return upfirdn2d(input, self.kernel, up=1, down=self.factor, pad=self.pad)


class Blur(nn.Module):
    """FIR low-pass with explicit padding (stylegan2.py:89-105)."""

    def __init__(self, kernel, pad, upsample_factor=1):
        super().__init__()
        taps = make_kernel(kernel)
        if upsample_factor > 1:
            taps = taps * (upsample_factor ** 2)
        self.register_buffer('kernel', taps)
        self.pad = pad

    def forward(self, input):
        return upfirdn2d(input, self.kernel, pad=self.pad)


class EqualConv2d(nn.Module):
    """Conv2d with equalised learning rate: N(0,1) weights scaled by 1/sqrt(fan_in) at run time (stylegan2.py:108-143)."""

    def __init__(self, in_channel, out_channel, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(out_channel, in_channel, kernel_size, kernel_size))
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.stride = stride
        self.padding = padding
        self.bias = nn.Parameter(torch.zeros(out_channel)) if bias else None

    def forward(self, input):
        if input.is_cuda and torch.is_grad_enabled():
            # same convolution; its derivatives of every order are the library's backward-data / backward-weight
            # primitives (op/conv_grad.py: PyTorch's generic conv double-backward costs R1 1.6 s per step at 1024^2)
            return conv_grad.conv2d(input, self.weight * self.scale, self.bias, self.stride, self.padding)
        return F.conv2d(input, self.weight * self.scale, bias=self.bias, stride=self.stride, padding=self.padding)

    def __repr__(self):
        o, i, k, _ = self.weight.shape
        return f'{self.__class__.__name__}({i}, {o}, {k}, stride={self.stride}, padding={self.padding})'


class EqualLinear(nn.Module):
    """Linear with equalised learning rate and optional fused leaky ReLU (stylegan2.py:146-180)."""

    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, lr_mul=1, activation=None):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(out_dim, in_dim).div_(lr_mul))
        self.bias = nn.Parameter(torch.full((out_dim,), float(bias_init))) if bias else None
        self.activation = activation
        self.scale = (1 / math.sqrt(in_dim)) * lr_mul
        self.lr_mul = lr_mul
        self._live = None     # set by op.live_weights.LiveWeights of the enclosing network

    def _scaled_params(self):
        """weight*scale and bias*lr_mul (stylegan2.py:165-175).  Inside the inference forward of a network that owns a
        LiveWeights table they were re-derived from the live parameters by that forward's single refresh launch (the
        reference re-multiplies every 512x512 modulation matrix on every call: 88 elementwise launches per 1024^2
        forward); anywhere else they are computed here.  Nothing survives a forward, so in-place `.data` updates
        (EMA accumulate, train_3_encoder.py:195-200) can never be missed."""
        lv = live(self)
        if lv is not None:
            return lv
        w, b = self.weight, self.bias
        return w * self.scale, (None if b is None else b * self.lr_mul)

    def forward(self, input):
        weight, bias = self._scaled_params()
        if self.activation:
            return fused_leaky_relu(F.linear(input, weight), bias)
        # Inference at per-rank batch sizes (the modulation of every StyledConv / ToRGB: 26 launches per 1024^2 forward, on
        # the critical path between the contractions): a matrix-vector product per sample on this repo's kernel (the BLAS
        # library serves 8 x 512 x 512 with a 16 x 16 macro-tile GEMM in 19 us).  Same sums up to the order of addition;
        # measured 376.6 / 378.3 vs 375.6 / 377.2 pairs/s in alternating launches on one box.
        if (input.is_cuda and not torch.is_grad_enabled() and input.dim() == 2 and input.shape[0] <= 64
                and input.dtype == torch.float32 and weight.dtype == torch.float32 and not torch.is_autocast_enabled()):
            return _native.equal_linear(input, weight, bias)
        return F.linear(input, weight, bias=bias)

    def __repr__(self):
        return f'{self.__class__.__name__}({self.weight.shape[1]}, {self.weight.shape[0]})'


class ScaledLeakyReLU(nn.Module):
    def __init__(self, negative_slope=0.2):
        super().__init__()
        self.negative_slope = negative_slope

    def forward(self, input):
        return F.leaky_relu(input, negative_slope=self.negative_slope) * _SQRT2


def _fir_pads(n_taps, kernel_size, upsample):
    """Blur padding around the strided conv (stylegan2.py:216-230, 705-709)."""
    if upsample:
        p = (n_taps - 2) - (kernel_size - 1)
        return (p + 1) // 2 + 1, p // 2 + 1
    p = (n_taps - 2) + (kernel_size - 1)
    return (p + 1) // 2, p // 2


class ModulatedConv2d(nn.Module):
    """Per-sample modulated (and demodulated) convolution (stylegan2.py:195-298).

    The reference multiplies the weight by the style per sample and runs a grouped conv.  Here the style
    multiplies the INPUT while it is staged into LDS and the demodulation coefficient scales the OUTPUT in
    the kernel epilogue, so one weight matrix serves the whole batch on the MFMA units (op/modconv.py).
    """

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, demodulate=True, upsample=False,
                 downsample=False, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        self.eps = 1e-8
        self.kernel_size = kernel_size
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.upsample = upsample
        self.downsample = downsample
        if upsample:
            self.blur = Blur(blur_kernel, pad=_fir_pads(len(blur_kernel), kernel_size, True), upsample_factor=2)
        if downsample:
            self.blur = Blur(blur_kernel, pad=_fir_pads(len(blur_kernel), kernel_size, False))
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.padding = kernel_size // 2
        self.weight = nn.Parameter(torch.randn(1, out_channel, in_channel, kernel_size, kernel_size))
        self.modulation = EqualLinear(style_dim, in_channel, bias_init=1)
        self.demodulate = demodulate
        self._live = None     # set by op.live_weights.LiveWeights of the enclosing network
        self._live_u = None   # likewise: the Winograd weight, for the wide plain layers only

    def __repr__(self):
        return (f'{self.__class__.__name__}({self.in_channel}, {self.out_channel}, {self.kernel_size}, '
                f'upsample={self.upsample}, downsample={self.downsample})')

    def mfma_weight(self):
        """wt[i][tap][o] = scale * weight[o][i][tap]: this forward's refreshed table entry, else derived now."""
        lv = live(self)
        if lv is not None:
            return lv[0]
        with torch.no_grad():
            return _native.modconv_weight_prep(self.weight.detach(), self.scale)

    def mfma_wsq(self):
        """Per-(o,i) sum of squared taps for the demodulation kernel (same rule as mfma_weight)."""
        lv = live(self)
        if lv is not None:
            return lv[1]
        with torch.no_grad():
            return _native.modconv_wsq(self.weight.detach())

    def wino_weight(self):
        """U = G (scale * weight) Gt [16, cout, cin]: this forward's refreshed table entry, or None (modconv2d_winograd
        then derives it from mfma_weight() on the spot)."""
        return live_u(self)

    def styles(self, style):
        return self.modulation(style)

    def forward(self, input, style, return_style_scalars=False):
        s = self.styles(style)
        hip = modconv.hip_conv_ok(input, self.weight)
        wt = self.mfma_weight() if hip else None
        if self.upsample:
            out = self.blur(modconv.modulated_conv2d(input, self.weight, s, wt, self.demodulate, 1, self.scale))
        elif self.downsample:
            out = modconv.modulated_conv2d(self.blur(input), self.weight, s, wt, self.demodulate, 2, self.scale)
        else:
            out = modconv.modulated_conv2d(input, self.weight, s, wt, self.demodulate, 0, self.scale)
        if return_style_scalars:
            return out, s.view(s.shape[0], 1, self.in_channel, 1, 1)
        return out


class _NoiseInjectionFunction(autograd.Function):
    """image + weight * noise with a cheaper and more accurate weight gradient.  Autograd's own rule materialises
    grad_out * noise at full [B,C,H,W] size (1 GB per layer at 1024^2, B=8) and sums ~10^8 signed fp32 terms into one
    scalar — heavy cancellation: measured 2e-3 relative error against float64, 10-20x the CPU reference's.  Here the
    channels are summed first (one read of grad_out, float64 accumulation) and the [B,1,H,W] result is contracted
    with the noise in float64.  The backward is made of differentiable ops, so it also serves create_graph=True."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, image, weight, noise):
        ctx.save_for_backward(weight, noise)
        return image + weight * noise

    @staticmethod
    @_amp_bwd
    def backward(ctx, go):
        weight, noise = ctx.saved_tensors
        g_weight = g_noise = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            csum = go.sum(1, keepdim=True, dtype=torch.float64)                   # [B,1,H,W]
            if ctx.needs_input_grad[1]:
                g_weight = (csum * noise).sum().to(go.dtype).reshape(weight.shape)
            if ctx.needs_input_grad[2]:
                g_noise = (csum * weight).to(go.dtype)
                if noise.shape[0] != go.shape[0]:
                    g_noise = g_noise.sum(0, keepdim=True)
        return go, g_weight, g_noise


class NoiseInjection(nn.Module):
    """image + weight * noise, fresh N(0,1) noise when none is given (stylegan2.py:301-312)."""

    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1))

    def forward(self, image, noise=None):
        if noise is None:
            b, _, h, w = image.shape
            noise = image.new_empty(b, 1, h, w).normal_()
        if image.is_cuda and image.dtype == torch.float32 and image.ndim == 4 and noise.shape[1] == 1:
            return _NoiseInjectionFunction.apply(image, self.weight, noise)
        return image + self.weight * noise


class ConstantInput(nn.Module):
    """Learned 4x4 constant repeated over the batch (stylegan2.py:315-329)."""

    def __init__(self, channel, size=4):
        super().__init__()
        self.input = nn.Parameter(torch.randn(1, channel, size, size))

    def forward(self, input):
        return self.input.repeat(input.shape[0], 1, 1, 1)


WINOGRAD = os.environ.get('FMGAN_NO_WINOGRAD', '0') != '1'   # Winograd F(2x2,3x3) form of the wide plain convs (inference)


def winograd_pays(batch, cin, cout, h, w):
    """Plain StyledConv layers served by the Winograd form (op/_native/conv.py: modconv2d_winograd) instead of the direct MFMA kernel.
    Measured at B = 8 (profiles/r03_winograd.md): 16^2..64^2 x 512 channels 1.6-1.9x, 128^2 x 256 channels 1.23x, 256^2 x 128
    channels 0.83x (its transforms move 4x the activation through HBM): wide layers of at most 128^2 only, with enough tiles
    for the 16 GEMMs to fill the chip."""
    if not WINOGRAD or _native.current_modconv_precision() != 'f32' or (h | w) & 1:
        return False
    return cin >= 256 and cout >= 256 and 16 <= h <= 128 and 16 <= w <= 128 and batch * (h // 2) * (w // 2) >= 512
FUSE_RGB = os.environ.get('FMGAN_NO_RGB_FUSE', '0') != '1'   # ToRGB in the preceding conv's epilogue (inference)
# Generator(comod=...): all styles + demodulation coefficients in two launches (op/style_bank.py) instead of per layer
STYLE_BANK = os.environ.get('FMGAN_NO_STYLE_BANK', '0') != '1'


def _fp32(fn, *args):
    """fn(*args); under autocast, with autocast off and every tensor (also inside a list) as float32: the fused inference
    path hands raw fp32 pointers to the library, and the style MLP would otherwise produce a bf16 vector (the training path
    gets this from its autograd Functions).  A Modulation passes as it is: the bank's results are fp32 already."""
    if not torch.is_autocast_enabled():
        return fn(*args)

    def f(a):
        if isinstance(a, list):
            return [f(x) for x in a]
        return a.float() if torch.is_tensor(a) else a
    with torch.autocast('cuda', enabled=False):
        return fn(*[f(a) for a in args])


def _modulation(conv, style):
    """Modulation of a ModulatedConv2d: `style` itself if it is one already (the enclosing Generator's style bank computed
    it for this forward), else from the latent column `style` by this layer's own two launches."""
    if isinstance(style, Modulation):
        return style
    s = conv.styles(style)
    if not conv.demodulate:
        return Modulation(s, None)
    lv = live(conv)     # (wt, wsq) refreshed by the enclosing network's forward, if any
    return Modulation(s, _native.modconv_demod(conv.weight, s, conv.scale, conv.eps, lv[1] if lv else None))


class StyledConv(nn.Module):
    """ModulatedConv2d -> NoiseInjection -> FusedLeakyReLU (stylegan2.py:332-376).

    When no autograd graph is being built the three steps after the contraction run inside the conv kernel's
    epilogue (plain conv) or in one elementwise pass (after the upsampling blur): the activation is written once
    instead of three times.
    """

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, upsample=False, blur_kernel=[1, 3, 3, 1],
                 demodulate=True):
        super().__init__()
        self.conv = ModulatedConv2d(in_channel, out_channel, kernel_size, style_dim, upsample=upsample,
                                    blur_kernel=blur_kernel, demodulate=demodulate)
        self.noise = NoiseInjection()
        self.activate = FusedLeakyReLU(out_channel)

    def _fused_upsample(self, input, s, demod, noise):
        """Transposed conv into a private intermediate [B,C,2H+1,2W+1], then blur + noise + bias + act in the blur's store.
        The intermediate is in the aligned-row layout: every dwordx4 load of the blur is 16-byte aligned (the contiguous
        2W+1-float rows never are).  It is released when this returns."""
        conv, act = self.conv, self.activate
        b, _, h, w = input.shape
        c = conv.out_channel
        pad0, pad1 = conv.blur.pad
        shape, off, ps, rs = _native.aligned_rows_shape(b, c, 2 * h + 1, 2 * w + 1, pad0)
        wt = conv.mfma_weight()

        def produce(buf):
            _native.modconv2d(input, wt, s, demod, 1, strided_out=(buf.data_ptr() + 4 * off, ps, rs))

        def consume(buf, out):
            # row-march / LDS-DMA ring for planes >= 64 wide, plane-tile (whole planes in LDS) for the 8^2..32^2 layers
            return _native.blur_noise_bias_act(buf.data_ptr() + 4 * off, input.device, b, c, 2 * h + 1, 2 * w + 1, ps, rs,
                                               conv.blur.kernel, (pad0, pad1), noise, self.noise.weight, act.bias,
                                               act.negative_slope, act.scale, out=out)
        nbytes = 4 * shape[0] * shape[1] * shape[2]
        ws = None
        if (placement.active() and nbytes >= placement.MIN_BYTES
                and _native.blur_noise_bias_act_serves(b, c, 2 * h + 1, 2 * w + 1, ps, rs, conv.blur.kernel.shape,
                                                       (pad0, pad1))):
            # the largest buffers of the forward: a persistent pair whose placement was selected by measurement
            # (op/placement.py: the same kernel runs at 4.85 or 5.17 TB/s depending on which two blocks it gets).
            # Only where the fused blur has a kernel for the shape: otherwise consume() launches nothing, the
            # selection would time a no-op and the persistent output would never be written.
            ws = placement.workspace(self, (b, c, h, w), shape, (b, c, 2 * h, 2 * w), input.device, produce, consume)
        if ws is not None:
            produce(ws.buf)
            if consume(ws.buf, ws.out) is None:
                raise RuntimeError('StyledConv: the fused blur declined a shape its selection reported as served')
            return ws.out
        buf = torch.empty(shape, dtype=torch.float32, device=input.device)
        produce(buf)
        out = consume(buf, None)
        if out is None:   # neither kernel serves it (planes > ~110^2 narrower than 64, FIRs wider than 4 taps): two passes
            out = _native.upfirdn2d_strided(buf.data_ptr() + 4 * off, input.device, b * c, 2 * h + 1, 2 * w + 1, ps,
                                            rs, conv.blur.kernel, pad0, pad1, pad0, pad1).view(b, c, 2 * h, 2 * w)
            out = _native.noise_bias_act(out, noise, self.noise.weight, act.bias, act.negative_slope, act.scale)
        return out

    def _fused(self, input, style, noise):
        conv, act = self.conv, self.activate
        s, demod = _modulation(conv, style)
        b, _, h, w = input.shape
        if noise is None:
            noise = input.new_empty(b, 1, *((2 * h, 2 * w) if conv.upsample else (h, w))).normal_()
        if conv.upsample:
            out = self._fused_upsample(input, s, demod, noise)
        elif winograd_pays(b, conv.in_channel, conv.out_channel, h, w):
            # 16 products per 2x2 output tile instead of 36 (own transform kernels around 16 batched library GEMMs): the
            # direct kernel is already at 0.84-0.88 of the fp32 matrix peak on these layers
            out = _native.modconv2d_winograd(input, conv.mfma_weight(), s, demod, noise=noise,
                                             noise_weight=self.noise.weight, bias=act.bias, fuse_act=True,
                                             alpha=act.negative_slope, act_scale=act.scale, u=conv.wino_weight())
        else:
            out = _native.modconv2d(input, conv.mfma_weight(), s, demod, 0, noise=noise,
                                    noise_weight=self.noise.weight, bias=act.bias, fuse_act=True,
                                    alpha=act.negative_slope, act_scale=act.scale)
        return out, s

    def rgb_fusable(self, x_shape, x):
        """Can this (plain) StyledConv take the following ToRGB into its epilogue for an input of this shape?"""
        conv = self.conv
        if conv.upsample or conv.downsample or torch.is_grad_enabled() or not modconv.hip_conv_ok(x, conv.weight):
            return False
        if _native.current_modconv_precision() != 'f32':     # the RGB epilogue exists on the fp32 MFMA kernel only
            return False
        b, _, h, w = x_shape
        return _native.modconv2d_rgb_fusable(b, conv.in_channel, conv.out_channel, h, w)

    def fused_with_rgb(self, input, style, noise, to_rgb, rgb_style, skip_up, keep_out):
        """StyledConv + ToRGB in one kernel (inference): returns (activation or None, rgb)."""
        return _fp32(self._fused_with_rgb, input, style, noise, to_rgb, rgb_style, skip_up, keep_out)

    def _fused_with_rgb(self, input, style, noise, to_rgb, rgb_style, skip_up, keep_out):
        conv, act = self.conv, self.activate
        s, demod = _modulation(conv, style)
        rgb_s = _modulation(to_rgb.conv, rgb_style).style
        if noise is None:
            noise = input.new_empty(input.shape[0], 1, input.shape[2], input.shape[3]).normal_()
        return _native.modconv2d_rgb(input, conv.mfma_weight(), s, demod, noise, self.noise.weight, act.bias,
                                     act.negative_slope, act.scale, to_rgb.conv.weight, rgb_s,
                                     to_rgb.bias, skip_up, to_rgb.conv.scale, keep_out)

    def forward(self, input, style, return_style_scalars=False, noise=None):
        """`style`: a latent column [B, D], or a Modulation (inference on the fused path only: it has no other consumer)."""
        fused = (not torch.is_grad_enabled()) and modconv.hip_conv_ok(input, self.conv.weight) and not self.conv.downsample
        if isinstance(style, Modulation) and not fused:
            raise RuntimeError('StyledConv: precomputed styles serve the fused inference path on float32 GPU tensors only')
        if fused:
            out, s = _fp32(self._fused, input, style, noise)
            if return_style_scalars:
                return out, s.view(s.shape[0], 1, self.conv.in_channel, 1, 1)
            return out
        if return_style_scalars:
            out, styles = self.conv(input, style, True)
        else:
            out = self.conv(input, style)
        out = self.activate(self.noise(out, noise=noise))
        return (out, styles) if return_style_scalars else out


class ToRGB(nn.Module):
    """1x1 modulated conv to RGB + bias + upsampled skip (stylegan2.py:379-404)."""

    def __init__(self, in_channel, style_dim, upsample=True, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        if upsample:
            self.upsample = Upsample(blur_kernel)
        self.conv = ModulatedConv2d(in_channel, 3, 1, style_dim, demodulate=False)
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))

    def forward(self, input, style, skip=None, return_style_scalars=False):
        s = _modulation(self.conv, style).style
        if skip is not None:
            skip = self.upsample(skip)
        out = modconv.to_rgb(input, self.conv.weight, s, self.bias, skip, self.conv.scale)
        if return_style_scalars:
            return out, s.view(s.shape[0], 1, self.conv.in_channel, 1, 1)
        return out


class _LatentStyles:
    """Style source of the synthesis loop, source(layer, i) -> the `style` argument of `layer`, which reads latent column
    i.  This one: the W+ tensor [B, columns, D] (training and plain inference)."""

    def __init__(self, latent):
        self.latent, self.columns = latent, latent.shape[1]

    def __call__(self, layer, i):
        return self.latent[:, i]


def _column_styles(provider):
    """Style source for W+ given one column at a time: provider(i), which may first wait for the stream that is still
    producing that column.  Used by Forward_Inference_3_Encoder to start the synthesis network before the last style heads
    of the encoder have finished."""
    return lambda layer, i: provider(i)


def _bank_styles(modulations):
    """Style source for {ModulatedConv2d: Modulation}, every layer's already computed by the style bank."""
    return lambda layer, i: modulations[layer.conv]


class Generator(nn.Module):
    """StyleGAN2 synthesis (+ mapping) network with the 3D-FM GAN extensions: external 4x4 input tensor, W+ input,
    in-forward path-length regulariser, RGB pyramid and style-scalar outputs (stylegan2.py:407-688)."""

    def __init__(self, size, style_dim, n_mlp, channel_multiplier=2, blur_kernel=[1, 3, 3, 1], lr_mlp=0.01,
                 generator_net_shape=None):
        super().__init__()
        self.size = size
        self.style_dim = style_dim
        mapping = [PixelNorm()]
        mapping += [EqualLinear(style_dim, style_dim, lr_mul=lr_mlp, activation='fused_lrelu') for _ in range(n_mlp)]
        self.style = nn.Sequential(*mapping)
        self.channels = _channel_table(channel_multiplier)
        self.log_size = int(math.log(size, 2))
        self.num_layers = (self.log_size - 2) * 2 + 1
        self.n_latent = self.log_size * 2 - 2

        # widths[j] = channels entering synthesis layer j; widths[-1] = channels leaving the last one.
        # generator_net_shape (pruned nets, Util/network_util.py:39-50) lists exactly that.
        if generator_net_shape is None:
            widths = [self.channels[4], self.channels[4]]
            for i in range(3, self.log_size + 1):
                widths += [self.channels[2 ** i]] * 2
        else:
            widths = list(generator_net_shape)

        self.input = ConstantInput(widths[0])
        self.conv1 = StyledConv(widths[0], widths[1], 3, style_dim, blur_kernel=blur_kernel)
        self.to_rgb1 = ToRGB(widths[1], style_dim, upsample=False)

        self.convs = nn.ModuleList()
        self.upsamples = nn.ModuleList()
        self.to_rgbs = nn.ModuleList()
        self.noises = nn.Module()
        for layer_idx in range(self.num_layers):
            res = 2 ** ((layer_idx + 5) // 2)
            self.noises.register_buffer(f'noise_{layer_idx}', torch.randn(1, 1, res, res))

        n_blocks = (self.log_size - 2) if generator_net_shape is None else (len(widths) // 2 - 1)
        for blk in range(1, n_blocks + 1):
            c_in, c_mid, c_out = widths[2 * blk - 1], widths[2 * blk], widths[2 * blk + 1]
            self.convs.append(StyledConv(c_in, c_mid, 3, style_dim, upsample=True, blur_kernel=blur_kernel))
            self.convs.append(StyledConv(c_mid, c_out, 3, style_dim, blur_kernel=blur_kernel))
            self.to_rgbs.append(ToRGB(c_out, style_dim))
        self._live_weights = None
        self._style_bank = None

    def make_noise(self):
        device = self.input.input.device
        noises = [torch.randn(1, 1, 4, 4, device=device)]
        for i in range(3, self.log_size + 1):
            noises += [torch.randn(1, 1, 2 ** i, 2 ** i, device=device) for _ in range(2)]
        return noises

    def mean_latent(self, n_latent):
        z = torch.randn(n_latent, self.style_dim, device=self.input.input.device)
        return self.style(z).mean(0, keepdim=True)

    def get_latent(self, input):
        return self.style(input)

    def _latents(self, styles, inject_index):
        """W+ tensor [B, n_latent, D] from one W/W+ batch or two W batches (style mixing), stylegan2.py:606-625."""
        if len(styles) < 2:
            w = styles[0]
            return w.unsqueeze(1).repeat(1, self.n_latent, 1) if w.ndim < 3 else w
        if inject_index is None:
            inject_index = random.randint(1, self.n_latent - 1)
        first = styles[0].unsqueeze(1).repeat(1, inject_index, 1)
        second = styles[1].unsqueeze(1).repeat(1, self.n_latent - inject_index, 1)
        return torch.cat([first, second], 1)

    def forward(self, *args, **kwargs):
        """Generator.forward of the reference (stylegan2.py:554-688; signature: _forward).  An inference call on the GPU
        first re-derives every scaled / MFMA-layout weight of the network from the live parameters in one launch
        (op/live_weights.py) and then runs the layers on those buffers."""
        if (not torch.is_grad_enabled()) and self.input.input.is_cuda:
            if self._live_weights is None:
                self._live_weights = LiveWeights(self)
            with self._live_weights.fresh(), placement.scope():
                return self._forward(*args, **kwargs)
        return self._forward(*args, **kwargs)

    def _forward(self, noise_z, return_latents=False, inject_index=None, truncation=1, truncation_latent=None,
                 latent_styles=None, input_is_latent=False, noise=None, randomize_noise=True,
                 use_external_input_tensor=False, external_input_tensor=None, PPL_regularize=False,
                 return_rgb_list=False, return_style_scalars=False, latent_columns=None, comod=None, comod_concat=None):
        """latent_columns (not in the reference): callable i -> W+[:, i] replacing latent_styles; inference only, with
        an external input tensor (see _column_styles).
        comod (not in the reference): (W [T,D], W+ [P,n_styles,D] with P in {1,T}, sliced columns or None for all),
        replacing latent_styles with latent[:, i] = W * W+[:, i] where sliced, W elsewhere — all known before the network
        starts, so the styles and demodulation coefficients of every layer come from the style bank's two launches
        (op/style_bank.py; STYLE_BANK = False / FMGAN_NO_STYLE_BANK=1: per layer, from the same columns).  Inference
        only, float32 GPU tensors, with an external input tensor of T samples or (the 2-encoder scheme's 'Multiplication'
        mode has none) the Generator's own ConstantInput for T samples.  The bank reads the LiveWeights buffers, so
        with STYLE_BANK on a Generator whose weights could not be refreshed (parameters that are not contiguous float32
        GPU tensors) raises RuntimeError rather than changing to the per-layer form unasked; STYLE_BANK = False serves it.
        comod_concat (not in the reference): (V [T,Dv], W+ [P,n_styles,Dw] with P in {1,T}), Dv + Dw = style_dim,
        replacing latent_styles with latent[:, i] = [V | W+[:, i]] for every column (the 2-encoder scheme's 'Concatenation'
        and 'Tensor Transform' modes, Util/network_util.py:264-282) — from the bank's concatenating launch, the
        concatenation never materialised, or (STYLE_BANK = False) per layer from each concatenated column.  Same
        restrictions as comod, and not together with it."""
        if comod is not None and comod_concat is not None:
            raise ValueError('comod and comod_concat are two forms of co-modulation: give one')

        def run(noise, external_input_tensor, *codes):
            source = self._style_source(noise_z, return_latents, inject_index, truncation, truncation_latent, latent_styles,
                                        input_is_latent, noise, randomize_noise, use_external_input_tensor,
                                        external_input_tensor, PPL_regularize, return_style_scalars, latent_columns,
                                        codes if comod is not None else None, codes if comod_concat is not None else None)
            return self._synthesis(*source, PPL_regularize, return_rgb_list, return_style_scalars)
        if comod is None and comod_concat is None:
            return run(noise, external_input_tensor)
        # the bank takes raw fp32 pointers, like the fused layers
        return _fp32(run, noise, external_input_tensor, *(comod if comod is not None else comod_concat))

    def _comod_styles(self, comod, external_input_tensor):
        """Style source of comod=(W, W+, sliced): the bank's result, or (STYLE_BANK = False) the columns one at a time."""
        w_r, w_plus, sliced = comod
        tensors = [t for t in (w_r, w_plus, external_input_tensor) if t is not None]   # no tensor: ConstantInput
        for t in tensors:
            _native.require_gpu(t, 'comod input')
        if (w_r.dim() != 2 or w_plus.dim() != 3 or w_plus.shape[0] not in (1, w_r.shape[0])
                or w_plus.shape[2] != w_r.shape[1] or w_plus.shape[1] < self.n_latent
                or (external_input_tensor is not None and external_input_tensor.shape[0] != w_r.shape[0])):
            raise ValueError('comod: W [T,D], W+ [1 or T, n_styles >= n_latent, D] and an external tensor of T samples')
        for t in tensors:
            _native.fp(t)           # float32 GPU tensors only: the kernels take raw pointers
        w_r, w_plus = w_r.contiguous(), w_plus.contiguous()
        cols = sliced_columns(sliced, self.n_latent, w_plus.shape[1])
        if STYLE_BANK:
            if self._live_weights is None or not self._live_weights.active:
                raise RuntimeError('comod: the style bank needs the Generator\'s refreshed weights (call the module, '
                                   'with float32 parameters on the GPU)')
            if getattr(self, '_style_bank', None) is None:
                self._style_bank = StyleBank(self)
            return _bank_styles(self._style_bank.run(w_r, w_plus, cols))
        cache = {}

        def column(i):
            if i not in cache:
                cache[i] = comod_column(w_r, w_plus[:, i], i, cols)
            return cache[i]
        return _column_styles(column)

    def _concat_styles(self, comod_concat, external_input_tensor):
        """Style source of comod_concat=(V, W+): the bank's result, or (STYLE_BANK = False) each concatenated column, built
        once, one at a time."""
        if len(comod_concat) != 2:
            raise ValueError('comod_concat: (V [T,Dv], W+ [1 or T, n_styles >= n_latent, Dw])')
        v, w_plus = comod_concat
        tensors = [t for t in (v, w_plus, external_input_tensor) if t is not None]     # no tensor: ConstantInput
        for t in tensors:
            _native.require_gpu(t, 'comod_concat input')
        if (v.dim() != 2 or w_plus.dim() != 3 or w_plus.shape[0] not in (1, v.shape[0])
                or v.shape[1] + w_plus.shape[2] != self.style_dim or w_plus.shape[1] < self.n_latent
                or (external_input_tensor is not None and external_input_tensor.shape[0] != v.shape[0])):
            raise ValueError('comod_concat: V [T,Dv], W+ [1 or T, n_styles >= n_latent, Dw] with Dv + Dw = style_dim and, '
                             'if any, an external tensor of T samples')
        for t in tensors:
            _native.fp(t)           # float32 GPU tensors only: the kernels take raw pointers
        v, w_plus = v.contiguous(), w_plus.contiguous()
        if STYLE_BANK:
            if self._live_weights is None or not self._live_weights.active:
                raise RuntimeError('comod_concat: the style bank needs the Generator\'s refreshed weights (call the '
                                   'module, with float32 parameters on the GPU)')
            if getattr(self, '_style_bank', None) is None:
                self._style_bank = StyleBank(self)
            return _bank_styles(self._style_bank.run_concat(v, w_plus))
        cache = {}

        def column(i):
            if i not in cache:
                cache[i] = concat_column(v, w_plus[:, i])
            return cache[i]
        return _column_styles(column)

    def _style_source(self, noise_z, return_latents, inject_index, truncation, truncation_latent, latent_styles,
                      input_is_latent, noise, randomize_noise, use_external_input_tensor, external_input_tensor,
                      PPL_regularize, return_style_scalars, latent_columns, comod, comod_concat=None):
        """(style source, noise of every layer, first activation) for the arguments of _forward."""
        plain = use_external_input_tensor and not (PPL_regularize or return_latents or return_style_scalars)
        frames = None           # co-modulation without an external tensor: samples of the Generator's own ConstantInput
        if comod is not None or comod_concat is not None:
            # the plain inference forward on the GPU: with the caller's input tensor, or with this Generator's constant
            # input (which then has to be where the kernels are: a Generator on the CPU has no such forward)
            served = not (PPL_regularize or return_latents or return_style_scalars) and (
                external_input_tensor is not None if use_external_input_tensor else self.input.input.is_cuda)
            if not served or torch.is_grad_enabled() or latent_columns is not None:
                raise ValueError(('comod' if comod is not None else 'comod_concat') +
                                 ' serves the plain inference forward (no_grad, external input tensor) only')
            tensor = external_input_tensor if use_external_input_tensor else None
            styles = self._comod_styles(comod, tensor) if comod is not None else self._concat_styles(comod_concat, tensor)
            if tensor is None:
                frames = (comod or comod_concat)[0]
        elif latent_columns is not None:
            if not plain:
                raise ValueError('latent_columns serves the plain inference forward only')
            styles = _column_styles(latent_columns)
        else:
            ws = latent_styles if input_is_latent else [self.style(z) for z in noise_z]
            if truncation < 1:
                ws = [truncation_latent + truncation * (w - truncation_latent) for w in ws]
            styles = _LatentStyles(self._latents(ws, inject_index))
        if noise is None:
            noise = [None if randomize_noise else getattr(self.noises, f'noise_{i}') for i in range(self.num_layers)]
        if use_external_input_tensor:
            assert external_input_tensor is not None
            return styles, noise, external_input_tensor
        return styles, noise, self.input(styles.latent if frames is None else frames)

    def _synthesis(self, styles, noise, out, PPL_regularize, return_rgb_list, return_style_scalars):
        """The synthesis network on the first activation `out`: layer L, reading latent column i, gets styles(L, i)."""
        scalars = []

        def run(layer, x, i, **kw):
            if return_style_scalars:
                y, s = layer(x, styles(layer, i), return_style_scalars=True, **kw)
                scalars.append(s)
                return y
            return layer(x, styles(layer, i), **kw)

        # Inference: the RGB branch (ToRGB + skip upsample, HBM-bound) of resolution r has no consumer until the
        # image is returned, so it runs on a side stream beside the MFMA-bound convs of resolution 2r.
        overlap = overlap_ok(out) and not return_style_scalars
        joins = []

        def rgb(layer, x, i, skip):
            if not overlap:
                return layer(x, styles(layer, i), skip)
            join, y = run_on(side, layer, x, styles(layer, i), skip)
            joins.append(join)
            return y

        if overlap:
            side, = side_streams(out.device, 1)
        out = run(self.conv1, out, 0, noise=noise[0])
        skip = rgb(self.to_rgb1, out, 1, None)
        rgbs = [skip]
        for blk, to_rgb in enumerate(self.to_rgbs):
            i = 1 + 2 * blk
            conv_a, conv_b = self.convs[2 * blk], self.convs[2 * blk + 1]
            b_, _, h_, w_ = out.shape
            # Inference, last resolution: its ToRGB cannot hide beside later convs (there are none) and is the only
            # consumer of conv_b's activation, so it rides in conv_b's epilogue and the [B,C,size,size] activation is
            # never written or re-read (2.1 GB of HBM traffic at 1024^2, B=8).  Lower resolutions keep the separate
            # ToRGB kernel: it overlaps the next resolution's MFMA-bound convs on the side stream (measured: fusing
            # those too is time-neutral on the conv and puts the RGB reduction on the critical path).
            last = blk + 1 == len(self.to_rgbs)
            if (FUSE_RGB and last and not return_style_scalars and not return_rgb_list
                    and conv_b.rgb_fusable((b_, 0, 2 * h_, 2 * w_), out)):
                if overlap:
                    join_up, skip_up = run_on(side, to_rgb.upsample, skip)
                    joins.append(join_up)
                else:
                    skip_up = to_rgb.upsample(skip)
                out = conv_a(out, styles(conv_a, i), noise=noise[i])
                if overlap:
                    join_up()
                out, skip = conv_b.fused_with_rgb(out, styles(conv_b, i + 1), noise[i + 1], to_rgb, styles(to_rgb, i + 2),
                                                  skip_up, keep_out=False)
                rgbs.append(skip)
                continue
            out = run(conv_a, out, i, noise=noise[i])
            out = run(conv_b, out, i + 1, noise=noise[i + 1])
            if return_style_scalars and i + 3 == styles.columns:   # style scalars of the last ToRGB only (:660-662)
                skip = run(to_rgb, out, i + 2, skip=skip)
            else:
                skip = rgb(to_rgb, out, i + 2, skip)
            rgbs.append(skip)
        for join in joins[-1:]:
            join()                      # the side stream is in order: joining its last launch joins all of them
        image = skip
        for r in rgbs[:-1]:
            if overlap:
                r.record_stream(torch.cuda.current_stream(image.device))

        if PPL_regularize:
            # path-length regulariser evaluated inside forward so it shards with the batch (stylegan2.py:683-688)
            probe = torch.randn_like(image) / math.sqrt(image.shape[2] * image.shape[3])
            grad, = autograd.grad(outputs=(image * probe).sum(), inputs=styles.latent, create_graph=True)
            return image, torch.sqrt(grad.pow(2).sum(2).mean(1))

        returns = rgbs if return_rgb_list else image
        return (returns, scalars) if return_style_scalars else returns


class ConvLayer(nn.Sequential):
    """[Blur] -> EqualConv2d -> [FusedLeakyReLU | ScaledLeakyReLU] (stylegan2.py:692-737)."""

    def __init__(self, in_channel, out_channel, kernel_size, downsample=False, blur_kernel=[1, 3, 3, 1], bias=True,
                 activate=True):
        layers = []
        if downsample:
            layers.append(Blur(blur_kernel, pad=_fir_pads(len(blur_kernel), kernel_size, False)))
            stride, self.padding = 2, 0
        else:
            stride, self.padding = 1, kernel_size // 2
        layers.append(EqualConv2d(in_channel, out_channel, kernel_size, padding=self.padding, stride=stride,
                                  bias=bias and not activate))
        if activate:
            layers.append(FusedLeakyReLU(out_channel) if bias else ScaledLeakyReLU(0.2))
        super().__init__(*layers)


class ResBlock(nn.Module):
    """(conv3x3 -> blur+conv3x3/2 + blur+conv1x1/2 skip) / sqrt(2) (stylegan2.py:740-759)."""

    def __init__(self, in_channel, out_channel, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        self.conv1 = ConvLayer(in_channel, in_channel, 3)
        self.conv2 = ConvLayer(in_channel, out_channel, 3, downsample=True)
        self.skip = ConvLayer(in_channel, out_channel, 1, downsample=True, activate=False, bias=False)

    def forward(self, input):
        return (self.conv2(self.conv1(input)) + self.skip(input)) / _SQRT2


class Discriminator(nn.Module):
    """StyleGAN2 residual discriminator with minibatch-stddev (stylegan2.py:762-820)."""

    def __init__(self, size, channel_multiplier=2, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        channels = _channel_table(channel_multiplier)
        log_size = int(math.log(size, 2))
        convs = [ConvLayer(3, channels[size], 1)]
        in_channel = channels[size]
        for i in range(log_size, 2, -1):
            out_channel = channels[2 ** (i - 1)]
            convs.append(ResBlock(in_channel, out_channel, blur_kernel))
            in_channel = out_channel
        self.convs = nn.Sequential(*convs)
        self.stddev_group = 4
        self.stddev_feat = 1
        self.final_conv = ConvLayer(in_channel + 1, channels[4], 3)
        self.final_linear = nn.Sequential(
            EqualLinear(channels[4] * 4 * 4, channels[4], activation='fused_lrelu'),
            EqualLinear(channels[4], 1),
        )

    def forward(self, input):
        out = self.convs(input)
        batch, channel, height, width = out.shape
        group = min(batch, self.stddev_group)
        # (the statistic is taken in fp32 also when the activations are 16-bit — a converted network, or autocast with
        # _native.activation_io('16'): a variance over 4 samples in bf16 keeps 2-3 digits; a no-op on fp32 activations)
        sd = out.float().view(group, -1, self.stddev_feat, channel // self.stddev_feat, height, width)
        sd = torch.sqrt(sd.var(0, unbiased=False) + 1e-8)
        sd = sd.mean([2, 3, 4], keepdims=True).squeeze(2).repeat(group, 1, height, width)
        out = self.final_conv(torch.cat([out, sd.to(out.dtype)], 1))
        return self.final_linear(out.view(batch, -1))
