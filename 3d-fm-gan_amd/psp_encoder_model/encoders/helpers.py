"""IR / IR-SE building blocks of the pSp W+ encoder (reference: psp_encoder_model/encoders/helpers.py).

Inference on the GPU (fused_body / fused_units): BN / SE / shortcut / add of the units run on the glue kernels of
csrc/encoder_glue.hip, and the units' 3x3 convolutions whose output is at least BODY_X3_MIN_OUT = 32 wide run on the
split-operand kernel family of csrc/conv3x3_x3.hip (three bf16 pieces per fp32 operand, fp32 accumulation) instead of
MIOpen's fp32 implicit GEMM: conv1 with the unit's PReLU in its epilogue, conv2 (stride 1 or 2) with a plain store,
channels_last in and out.  At a 256^2 photo these are both convolutions of units 0-5 and conv1 of unit 6; the 16^2 ones
keep MIOpen + aten PReLU.  The rule is body_x3_serves, the switch BODY_X3 / FMGAN_PSP_BODY_X3=0
(profiles/psp_body_x3.md)."""
import os
from collections import namedtuple

import torch
import torch.nn.functional as F
from torch import nn

from op._native import amp_fwd as _amp_fwd, amp_bwd as _amp_bwd
from torch.nn import (AdaptiveAvgPool2d, BatchNorm2d, Conv2d, MaxPool2d, Module, ReLU, Sequential, Sigmoid)


class _PReLUFunction(torch.autograd.Function):
    """aten's prelu forward with the backward on the HIP kernel fmgan_prelu_backward_f32 (one pass over x and grad, the
    slope gradient as per-block partial sums): aten's prelu_backward writes two full-size tensors through a multi-output
    elementwise kernel that does not vectorise on NHWC data — 965 us per call at [16,64,256,256], 6.5 % of the
    forward+backward of the 3-encoder path.  When a graph of the backward is requested (create_graph=True) the same
    formulas run as differentiable torch ops."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return F.prelu(x, weight)

    @staticmethod
    @_amp_bwd
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        if not torch.is_grad_enabled():
            from op import _native
            n, c, h, w = x.shape
            x2 = x.permute(0, 2, 3, 1)
            g2 = grad.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
            if x2.is_contiguous() and g2.is_contiguous():
                res = _native.prelu_backward(x2.reshape(-1, c), g2.reshape(-1, c), weight.contiguous())
                if res is not None:
                    gx, gw = res
                    return gx.view(n, h, w, c).permute(0, 3, 1, 2), gw
        neg = x <= 0
        a = weight.view(1, -1, 1, 1)
        return torch.where(neg, grad * a, grad), (grad * x * neg).sum((0, 2, 3))


class PReLU(nn.PReLU):
    """nn.PReLU(depth) (same parameter, same state_dict) whose training-time backward on NHWC float32 GPU activations
    runs on the HIP kernel above; everything else is nn.PReLU."""

    def forward(self, input):
        if (input.is_cuda and input.dtype == torch.float32 and input.dim() == 4 and torch.is_grad_enabled()
                and (input.requires_grad or self.weight.requires_grad) and self.weight.numel() == input.shape[1]
                and self.weight.numel() % 4 == 0
                and input.is_contiguous(memory_format=torch.channels_last) and not input.is_contiguous()):
            return _PReLUFunction.apply(input, self.weight)
        return super().forward(input)


class Flatten(Module):
    def forward(self, input):
        return input.view(input.size(0), -1)


def l2_norm(input, axis=1):
    return torch.div(input, torch.norm(input, 2, axis, True))


class Bottleneck(namedtuple('Block', ['in_channel', 'depth', 'stride'])):
    """(in_channel, depth, stride) of one residual unit."""


def get_block(in_channel, depth, num_units, stride=2):
    return [Bottleneck(in_channel, depth, stride)] + [Bottleneck(depth, depth, 1) for _ in range(num_units - 1)]


_UNITS = {18: (2, 2, 2, 2), 50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}


def get_blocks(num_layers):
    """Unit layout per stage (helpers.py:38-73): widths 64/128/256/512, first unit of each stage has stride 2."""
    if num_layers not in _UNITS:
        raise ValueError(f'Invalid number of layers: {num_layers}. Must be one of [18, 50, 100, 152]')
    widths = (64, 64, 128, 256, 512)
    return [get_block(widths[i], widths[i + 1], n) for i, n in enumerate(_UNITS[num_layers])]


class SEModule(Module):
    """Squeeze-and-excitation gate (helpers.py:76-92)."""

    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = AdaptiveAvgPool2d(1)
        self.fc1 = Conv2d(channels, channels // reduction, kernel_size=1, padding=0, bias=False)
        self.relu = ReLU(inplace=True)
        self.fc2 = Conv2d(channels // reduction, channels, kernel_size=1, padding=0, bias=False)
        self.sigmoid = Sigmoid()

    def forward(self, x):
        gate = self.sigmoid(self.fc2(self.relu(self.fc1(self.avg_pool(x)))))
        return x * gate


def _shortcut(in_channel, depth, stride):
    if in_channel == depth:
        return MaxPool2d(1, stride)
    return Sequential(Conv2d(in_channel, depth, (1, 1), stride, bias=False), BatchNorm2d(depth))


class bottleneck_IR(Module):
    """BN-conv3x3-PReLU-conv3x3(stride)-BN + shortcut (helpers.py:95-114)."""

    def __init__(self, in_channel, depth, stride):
        super().__init__()
        self.shortcut_layer = _shortcut(in_channel, depth, stride)
        self.res_layer = Sequential(BatchNorm2d(in_channel),
                                    Conv2d(in_channel, depth, (3, 3), (1, 1), 1, bias=False), PReLU(depth),
                                    Conv2d(depth, depth, (3, 3), stride, 1, bias=False), BatchNorm2d(depth))

    def forward(self, x):
        return self.res_layer(x) + self.shortcut_layer(x)


class bottleneck_IR_SE(Module):
    """bottleneck_IR with an SE gate at the end of the residual branch (helpers.py:117-139)."""

    def __init__(self, in_channel, depth, stride):
        super().__init__()
        self.shortcut_layer = _shortcut(in_channel, depth, stride)
        self.res_layer = Sequential(BatchNorm2d(in_channel),
                                    Conv2d(in_channel, depth, (3, 3), (1, 1), 1, bias=False), PReLU(depth),
                                    Conv2d(depth, depth, (3, 3), stride, 1, bias=False), BatchNorm2d(depth),
                                    SEModule(depth, 16))

    def forward(self, x):
        return self.res_layer(x) + self.shortcut_layer(x)


# ----------------------------------------------------------------------------- inference body on the fused glue kernels
# Inference on the GPU (no_grad, fp32, channels_last): everything between a unit's MIOpen convolutions except the PReLU
# between its two 3x3 convolutions runs on four HIP kernels (csrc/encoder_glue.hip) — per unit PReLU, se_pool, se_gate and
# ir_tail instead of 11-12 aten / MIOpen launches, and one bn_prelu after the input convolution.  Every BatchNorm is
# evaluated in-kernel from the module's live vectors on every launch; modules, state_dict names and the training path
# are untouched.  FMGAN_NO_ENCODER_FUSE=1 (or ENCODER_FUSE = False) keeps the module path.
ENCODER_FUSE = os.environ.get('FMGAN_NO_ENCODER_FUSE', '0') != '1'
# On that path the units' 3x3 convolutions themselves run on the split-operand contraction of csrc/conv3x3_x3.hip
# (conv3x3_mfma_bf16x3: three bf16 pieces per fp32 operand, fp32 accumulation, fixed summation order) reading and writing
# channels_last storage: conv1 with the PReLU in its epilogue (the aten PReLU pass goes), conv2 (stride 1 or 2) with a
# plain store.  Which layers: body_x3_serves — every 3x3 convolution whose OUTPUT is at least BODY_X3_MIN_OUT wide (the
# kernel's position tile is 32 columns; profiles/psp_body_x3.md has the per-shape measurement against MIOpen): at a
# 256^2 photo units 0-5 and conv1 of unit 6, thirteen of the sixteen; the 16^2 ones stay on MIOpen's fp32 implicit GEMM
# followed by aten PReLU, exactly as before.  FMGAN_PSP_BODY_X3=0 (or BODY_X3 = False) gives MIOpen back everywhere.
BODY_X3 = os.environ.get('FMGAN_PSP_BODY_X3', '1') == '1'
BODY_X3_MIN_OUT = 32


class _NotServed(Exception):
    """A glue kernel declined a shape: the caller runs the modules instead."""


def _served(res):
    if res is None:
        raise _NotServed
    return res


def _bn(m):
    return m.running_mean, m.running_var, m.weight, m.bias, m.eps


def _bn_fusable(m, c):
    return (isinstance(m, BatchNorm2d) and not m.training and m.running_mean is not None and m.weight is not None
            and m.num_features == c and m.weight.dtype == torch.float32 and m.running_mean.dtype == torch.float32)


def _width_fusable(c):
    return c % 4 == 0 and c <= 1024


def _unit_fusable(unit):
    if not isinstance(unit, (bottleneck_IR, bottleneck_IR_SE)):
        return False
    res, sc = unit.res_layer, unit.shortcut_layer
    cin, depth = res[1].in_channels, res[3].out_channels
    if not (_width_fusable(cin) and _width_fusable(depth) and _bn_fusable(res[0], cin) and _bn_fusable(res[4], depth)
            and res[2].weight.numel() == depth):
        return False
    if len(res) == 6 and res[5].fc1.out_channels > 256:
        return False
    if isinstance(sc, MaxPool2d):
        return sc.kernel_size == 1 and sc.padding == 0 and sc.dilation == 1 and isinstance(sc.stride, int)
    return _bn_fusable(sc[1], depth)


def _input_fusable(x):
    return (ENCODER_FUSE and not torch.is_grad_enabled() and not torch.is_autocast_enabled() and x.is_cuda
            and x.dtype == torch.float32 and x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous())


def body_x3_serves(conv, x):
    """Does this 3x3 convolution of a unit run on _native.conv3x3_bf16x3 for the channels_last activation x?  The per-shape
    rule of the body, in one place: the switch, a plain 3x3 / pad 1 / stride 1 or 2 convolution without bias, an output
    at least BODY_X3_MIN_OUT wide, and the library's own query."""
    from op import _native
    if not (BODY_X3 and isinstance(conv, Conv2d) and conv.kernel_size == (3, 3) and conv.padding == (1, 1)
            and conv.stride in ((1, 1), (2, 2)) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.weight.dtype == torch.float32 and _native.nhwc_dense(x) and x.shape[1] == conv.in_channels):
        return False
    stride = conv.stride[0]
    if (x.shape[3] - 1) // stride + 1 < BODY_X3_MIN_OUT:
        return False
    return _native.conv3x3_bf16x3_supported(x.shape[0], conv.in_channels, conv.out_channels, x.shape[2], x.shape[3],
                                            stride, True)


def _unit_convs(res, xn):
    """conv1 -> PReLU -> conv2 of a unit on xn = BN_in(x): each convolution on the split-operand kernel where
    body_x3_serves says so (conv1 with the PReLU in its epilogue), on MIOpen (+ aten PReLU) otherwise."""
    from op import _native
    from op.live_weights import split_conv_weight
    conv1, act, conv2 = res[1], res[2], res[3]
    if body_x3_serves(conv1, xn):
        r = _native.conv3x3_bf16x3(xn, split_conv_weight(conv1), conv1.out_channels, conv1.stride[0], 'prelu', act.weight,
                                   channels_last=True)
        if r is None:
            raise RuntimeError('conv3x3_bf16x3 declined a shape its query accepted')
    else:
        r = act(conv1(xn))
    if body_x3_serves(conv2, r):
        r2 = _native.conv3x3_bf16x3(r, split_conv_weight(conv2), conv2.out_channels, conv2.stride[0], None,
                                    channels_last=True)
        if r2 is None:
            raise RuntimeError('conv3x3_bf16x3 declined a shape its query accepted')
        return r2
    return conv2(r)


def _fused_unit(unit, x, xn, bn_next, sub=None):
    """One unit on the glue kernels.  x: the unit's input, xn = BN_in(x), sub: x already subsampled by the unit's
    MaxPool2d(1, stride) shortcut (x may then be None).  Returns (out, bn_next(out) or None)."""
    from op import _native
    res, sc = unit.res_layer, unit.shortcut_layer
    r = _unit_convs(res, xn)
    gate = None
    if len(res) == 6:
        se = res[5]
        partial = _served(_native.se_pool(r))
        gate = _served(_native.se_gate(partial, r.shape[2] * r.shape[3], _bn(res[4]), se.fc1.weight, se.fc2.weight))
    if not isinstance(sc, MaxPool2d):
        return _served(_native.ir_tail(r, _bn(res[4]), gate, sc[0](x), 1, _bn(sc[1]), bn_next))
    if sub is not None:
        return _served(_native.ir_tail(r, _bn(res[4]), gate, sub, 1, None, bn_next))
    return _served(_native.ir_tail(r, _bn(res[4]), gate, x, sc.stride, None, bn_next))


def _fused_units(body, x, xn, sub, taps):
    feats = {}
    for i, unit in enumerate(body):
        bn_next = _bn(body[i + 1].res_layer[0]) if i + 1 < len(body) else None
        x, xn = _fused_unit(unit, x, xn, bn_next, sub)
        sub = None
        if i in taps:
            feats[i] = x
    return x, feats


def fused_units(body, x, taps=()):
    """The units of `body` (a Sequential of bottleneck_IR / bottleneck_IR_SE) on the glue kernels: (output, {tap index:
    that unit's output}), or None when the fused path does not apply (training, autograd, CPU, NCHW, autocast, a width the
    kernels do not serve): the caller then runs the modules.  The first unit's BN_in runs as a module here."""
    if not (_input_fusable(x) and len(body) > 0 and all(_unit_fusable(u) for u in body)):
        return None
    try:
        return _fused_units(body, x, body[0].res_layer[0](x), None, taps)
    except _NotServed:
        return None


def fused_body(input_layer, body, x, taps=()):
    """input_layer (conv, BatchNorm2d, PReLU) and the units of `body` on the glue kernels; as fused_units.  The input
    layer's bn_prelu also writes the first unit's BN_in and, when that unit's shortcut is MaxPool2d(1, stride), its
    subsampled shortcut — the full-size activation itself is then never written."""
    from op import _native
    if not (_input_fusable(x) and len(body) > 0 and all(_unit_fusable(u) for u in body) and len(input_layer) == 3):
        return None
    conv, bn, act = input_layer
    c = conv.out_channels
    if not (isinstance(conv, Conv2d) and _width_fusable(c) and _bn_fusable(bn, c) and isinstance(act, nn.PReLU)
            and act.weight.numel() == c and body[0].res_layer[1].in_channels == c):
        return None
    pool = body[0].shortcut_layer
    stride = pool.stride if isinstance(pool, MaxPool2d) else 0
    try:
        y, yn, sub = _served(_native.bn_prelu(conv(x), _bn(bn), act.weight, want_y=stride == 0,
                                              bn_next=_bn(body[0].res_layer[0]), sub_stride=stride))
        return _fused_units(body, y, yn, sub, taps)
    except _NotServed:
        return None
