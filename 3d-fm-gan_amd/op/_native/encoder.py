"""The pSp encoder body's fused BN / PReLU / SE / residual stages (inference): csrc/encoder_glue.hip."""
import torch

from .core import fp, launching, lib, nhwc_dense, _nhwc_empty, require_gpu, served


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
