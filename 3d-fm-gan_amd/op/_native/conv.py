"""The modulated convolution and what feeds it: csrc/modconv_prep.hip, modconv_fwd.hip, modconv_bf16.hip,
conv3x3_x3.hip, modconv_wgrad.hip, winograd.hip, torgb.hip, linear.hip, style_bank.hip."""
import ctypes

import torch

from .core import ambient, check, fp, launching, lib, nhwc_dense, _noise_args, on_device, ptr, require_gpu, served


# ----------------------------------------------------------------------------- csrc/modconv_prep.hip
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


# ----------------------------------------------------------------------------- what the launches share
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


class modconv_precision(ambient):
    """`with modconv_precision('bf16'):` — every modconv2d call inside (forward and data-gradient contractions of the
    modulated conv) whose shape the bf16 kernel serves runs on v_mfma_f32_32x32x16_bf16; the rest stay fp32."""
    values, text = ('f32', 'bf16', 'bf16x3'), "precision must be 'f32', 'bf16' or 'bf16x3'"
    scope, var = globals(), '_mc_precision'


def current_modconv_precision():
    return _mc_precision


# ----------------------------------------------------------------------------- csrc/modconv_fwd.hip
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


# ----------------------------------------------------------------------------- csrc/modconv_bf16.hip
def modconv_weight_to_bf16(wt):
    """fp32 MFMA layout wt [cin, taps, cout] (modconv_weight_prep) -> bf16 operand image (opaque int16 tensor)."""
    cin, taps, cout = wt.shape
    nbytes = lib().fmgan_modconv_weight_bf16_bytes(cin, cout, taps)
    wtb = torch.empty(nbytes // 2, dtype=torch.int16, device=wt.device)
    with on_device(wt) as stream:
        check(lib().fmgan_modconv_weight_to_bf16(fp(wt), ptr(wtb), cin, cout, taps, stream), 'modconv_weight_to_bf16')
    return wtb


def modconv_weight_to_bf16x3(wt):
    """fp32 MFMA layout wt [cin, taps, cout] -> its three bf16 operand images (hi, mid, lo) in one opaque tensor."""
    cin, taps, cout = wt.shape
    nbytes = lib().fmgan_modconv_weight_bf16x3_bytes(cin, cout, taps)
    wts = torch.empty(nbytes // 2, dtype=torch.int16, device=wt.device)
    with on_device(wt) as stream:
        check(lib().fmgan_modconv_weight_to_bf16x3(fp(wt), ptr(wts), cin, cout, taps, stream), 'modconv_weight_to_bf16x3')
    return wts


def conv_weight_to_bf16x3(weight, bracket='conv_weight_bf16x3'):
    """A Conv2d weight [cout, cin, 3, 3] (any memory format) -> the split-operand image of conv3x3s2_bf16x3: the
    [cin, 9, cout] order, then modconv_weight_to_bf16x3.  One bracket round the two steps, named `bracket`
    ('conv_weight_bf16x3'; the heads' narrow-tile convolutions build theirs under 'conv_tail_weight_bf16x3')."""
    require_gpu(weight, 'weight')
    cout, cin, kh, kw = weight.shape
    with launching(weight, bracket, (cout, cin, kh * kw)):
        wt = weight.detach().permute(1, 2, 3, 0).reshape(cin, kh * kw, cout).contiguous()
        return modconv_weight_to_bf16x3(wt)


# ----------------------------------------------------------------------------- csrc/conv3x3_x3.hip
def conv3x3s2_bf16x3_supported(batch, cin, cout, h, w):
    return bool(lib().fmgan_conv3x3s2_bf16x3_supported(int(batch), int(cin), int(cout), int(h), int(w)))


def conv3x3s2_bf16x3(x, wts, bias, cout, alpha=0.01, channels_last=False):
    """LeakyReLU(conv3x3(x, stride 2, pad 1) + bias) with fp32 operands split into three bf16 pieces (fp32 accumulation).
    x [B,cin,H,W] f32 NCHW-contiguous or dense channels_last storage (read as it is, same bits), wts =
    conv_weight_to_bf16x3(weight), bias [cout] or None.  Returns
    [B,cout,(H-1)//2+1,(W-1)//2+1] — NCHW-contiguous, or in channels_last storage (written so by the kernel: what the
    MIOpen tail of a style head reads) — or None where the library declines the shape."""
    require_gpu(x, 'input')
    in_nhwc = _c3_input_layout('conv3x3s2_bf16x3', x)
    b, cin, h, w = x.shape
    out = torch.empty((b, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=x.device,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    with launching(x, 'conv3x3s2_bf16x3', (b, cin, cout, h, w)) as stream:
        if in_nhwc:     # the same kernel reading channels_last storage (same bits), through the family's entry point
            st = lib().fmgan_conv3x3_bf16x3_f32(fp(x), ptr(wts), fp(bias), fp(out), b, cin, cout, h, w, 2, 1,
                                                int(bool(channels_last)), C3_EPILOGUES['lrelu'], float(alpha), stream)
        else:
            st = lib().fmgan_conv3x3s2_bf16x3_f32(fp(x), ptr(wts), fp(bias), fp(out), b, cin, cout, h, w, float(alpha),
                                                  int(bool(channels_last)), stream)
    return out if served(st, 'conv3x3s2_bf16x3') else None


C3_EPILOGUES = {None: 0, 'lrelu': 1, 'prelu': 2}        # include/fmgan_hip.h, fmgan_conv3x3_bf16x3_f32


def _c3_input_layout(what, x):
    """0 for an NCHW-contiguous input, 1 for dense channels_last storage (a tensor that is both, C = 1 or H = W = 1,
    counts as NCHW: the two layouts then coincide); anything else is refused."""
    if x.is_contiguous():
        return 0
    if nhwc_dense(x):
        return 1
    raise RuntimeError(f'{what}: input must be NCHW-contiguous or dense channels_last, got strides {x.stride()}')


def conv3x3_bf16x3_supported(batch, cin, cout, h, w, stride=1, channels_last_in=False):
    return bool(lib().fmgan_conv3x3_bf16x3_supported(int(batch), int(cin), int(cout), int(h), int(w), int(stride),
                                                     int(bool(channels_last_in))))


def conv3x3_bf16x3(x, wts, cout, stride=1, epilogue=None, aux=None, alpha=0.01, channels_last=False):
    """conv3x3(x, stride 1 or 2, pad 1) through one epilogue, fp32 operands split into three bf16 pieces (fp32
    accumulation): epilogue None: the plain convolution; 'lrelu': LeakyReLU(conv + aux) with aux = bias [cout] or None;
    'prelu': conv > 0 ? conv : aux * conv with aux = the PReLU slope [cout].  x [B,cin,H,W] f32, NCHW-contiguous or dense
    channels_last storage (read as it is); wts = conv_weight_to_bf16x3(weight).  Returns [B,cout,(H-1)//stride+1,
    (W-1)//stride+1], NCHW-contiguous or (channels_last=True) written in channels_last storage, or None where the library
    declines the shape.  Launch bracket 'conv3x3_bf16x3' with info (b, cin, cout, h, w, stride, epilogue code)."""
    require_gpu(x, 'input')
    in_nhwc = _c3_input_layout('conv3x3_bf16x3', x)
    epi = C3_EPILOGUES[epilogue]
    if epilogue == 'prelu' and (aux is None or aux.numel() != cout):
        raise RuntimeError('conv3x3_bf16x3: the prelu epilogue needs one slope per output channel')
    if aux is not None:
        aux = aux.contiguous()
    stride = int(stride)
    b, cin, h, w = x.shape
    out = torch.empty((b, cout, (h - 1) // max(stride, 1) + 1, (w - 1) // max(stride, 1) + 1), dtype=torch.float32,
                      device=x.device, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    with launching(x, 'conv3x3_bf16x3', (b, cin, cout, h, w, stride, epi)) as stream:
        st = lib().fmgan_conv3x3_bf16x3_f32(fp(x), ptr(wts), fp(aux), fp(out), b, cin, cout, h, w, stride, in_nhwc,
                                            int(bool(channels_last)), epi, float(alpha), stream)
    return out if served(st, 'conv3x3_bf16x3') else None


def conv3x3_tail_bf16x3_select(batch, cin, cout, h, w):
    """16 or 8: the tile width of conv3x3_tail_bf16x3 that serves the shape (stride-2 output 9 .. 16 or 5 .. 8 wide);
    otherwise the negative status its launch returns (FMGAN_EUNSUPPORTED, FMGAN_EINVAL).  Host logic, no device."""
    return int(lib().fmgan_conv3x3_tail_bf16x3_select(int(batch), int(cin), int(cout), int(h), int(w)))


def conv3x3_tail_bf16x3(x, wts, bias, cout, alpha=0.01, channels_last=True):
    """LeakyReLU(conv3x3(x, stride 2, pad 1) + bias) for outputs 5 .. 16 wide, on the narrow-tile members of the
    split-operand family (the bits of conv3x3_bf16x3(x, wts, cout, 2, 'lrelu', bias) on finite operands).  x [B,cin,H,W]
    f32 in dense channels_last storage, cin % 4 == 0; wts = conv_weight_to_bf16x3(weight); bias [cout] or None.  Returns
    [B,cout,(H-1)//2+1,(W-1)//2+1] written in channels_last storage (channels_last=False: NCHW-contiguous), or None
    where the library declines the shape.  Launch bracket 'conv3x3_tail_bf16x3' with info (b, cin, cout, h, w)."""
    require_gpu(x, 'input')
    if not nhwc_dense(x):
        raise RuntimeError(f'conv3x3_tail_bf16x3: input must be dense channels_last, got strides {x.stride()}')
    b, cin, h, w = x.shape
    out = torch.empty((b, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=x.device,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    with launching(x, 'conv3x3_tail_bf16x3', (b, cin, cout, h, w)) as stream:
        st = lib().fmgan_conv3x3_tail_bf16x3_f32(fp(x), ptr(wts), fp(bias), fp(out), b, cin, cout, h, w, float(alpha),
                                                 int(bool(channels_last)), stream)
    return out if served(st, 'conv3x3_tail_bf16x3') else None


# ----------------------------------------------------------------------------- csrc/modconv_wgrad.hip
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


def modconv_wgrad_select(batch, cin, cout, h, w, mode=0, aligned16=True):
    """(family, TW, SP, ksplit, tiles_per_split, ntiles, vec): the kernel (family 32 or 64: its channel tile; 64 is
    modconv_wgrad64_f32<log2 TW, SP>), the split over pixel tiles and the staging path (vec: 16-byte loads) that the library's
    weight-gradient launch takes for this shape, from the launch's own plan — host logic, no device needed.  aligned16: the
    unshifted operand (go; x in mode 1) is 16-byte aligned.  All zeros where the library declines the shape; raises as the
    launch would for arguments it refuses."""
    v = [ctypes.c_int() for _ in range(7)]
    st = lib().fmgan_modconv_wgrad_select(int(batch), int(cin), int(cout), int(h), int(w), int(mode), int(bool(aligned16)),
                                          *[ctypes.byref(c) for c in v])
    served(st, 'modconv_wgrad_select')
    family, tw, sp, ks, tps, ntiles, vec = (c.value for c in v)
    return family, tw, sp, ks, tps, ntiles, bool(vec)


# ----------------------------------------------------------------------------- csrc/winograd.hip
def wino_select(transform, batch, c, h, w, *tensors):
    """Which kernel wino_input (transform 'input') or wino_output ('output', c = cout) takes for these sizes: 'strip' (one
    thread per four horizontally adjacent tiles, 16-byte accesses) or 'tile' (one thread per tile) — the launch's own rule,
    host logic.  tensors: what the launch reads through 16-byte accesses (x; M and the noise plane) — None entries are
    skipped; the transform's own V / out are fresh allocations and always aligned.  Raises as the launch would for sizes it
    refuses."""
    aligned = all(t.data_ptr() % 16 == 0 for t in tensors if t is not None)
    k = lib().fmgan_wino_select(('input', 'output').index(transform), int(batch), int(c), int(h), int(w), int(aligned))
    check(min(k, 0), 'wino_select')
    return ('tile', 'strip')[k]


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


# ----------------------------------------------------------------------------- csrc/torgb.hip
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


# ----------------------------------------------------------------------------- csrc/linear.hip
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


# ----------------------------------------------------------------------------- csrc/style_bank.hip
def style_bank(table, n_entries, w, wplus, styles_out):
    """Every table entry's style in one launch (op/style_bank.py builds the table): w [T,D], wplus [P,n_styles,D] with
    P in {1, T}, styles_out flat f32 of T * sum(cin) elements."""
    if w.dim() != 2 or wplus.dim() != 3 or wplus.shape[2] != w.shape[1] or not (w.is_contiguous() and wplus.is_contiguous()):
        raise RuntimeError(f'style_bank: W {tuple(w.shape)} / W+ {tuple(wplus.shape)} must be contiguous [T,D] / [P,n,D]')
    with on_device(w) as stream:
        check(lib().fmgan_style_bank_f32(fp(table.view(torch.float32)), n_entries, fp(w), fp(wplus), wplus.shape[0],
                                         w.shape[0], w.shape[1], fp(styles_out), stream), 'style_bank')


def style_bank_concat(table, n_entries, v, wplus, styles_out):
    """Every table entry's style of the concatenating co-modulation in one launch: x = [v | wplus[:, col]] over each
    entry's [cin, Dv + Dw] matrix; v [T,Dv], wplus [P,n_styles,Dw] with P in {1, T}, styles_out as for style_bank()."""
    if v.dim() != 2 or wplus.dim() != 3 or not (v.is_contiguous() and wplus.is_contiguous()):
        raise RuntimeError(f'style_bank_concat: V {tuple(v.shape)} / W+ {tuple(wplus.shape)} must be contiguous [T,Dv] / '
                           f'[P,n,Dw]')
    with on_device(v) as stream:
        check(lib().fmgan_style_bank_concat_f32(fp(table.view(torch.float32)), n_entries, fp(v), fp(wplus), wplus.shape[0],
                                                v.shape[0], v.shape[1], wplus.shape[2], fp(styles_out), stream),
              'style_bank_concat')


def demod_bank(table, n_entries, styles, batch, demod_out):
    """Every demodulated table entry's coefficients in one launch, from the flat styles of style_bank()."""
    with on_device(styles) as stream:
        check(lib().fmgan_demod_bank_f32(fp(table.view(torch.float32)), n_entries, fp(styles), batch, fp(demod_out), stream),
              'demod_bank')
