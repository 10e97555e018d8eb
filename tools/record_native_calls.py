#!/usr/bin/env python3
"""Record every call into libfmgan_hip.so and every observer event of a fixed, seeded workload, as JSON.

    python tools/record_native_calls.py OUT.json

For refactors of op/_native: run it on the commit before and on the commit after and compare the two files — the same
entry points with the same arguments in the same order, bracketed by the same (name, info) events, is the same work on the
GPU.  The workload calls every public wrapper of op/_native at least once (through its op/*.py module where it has one),
at the smallest case of the wrapper's test table.  After the first _native.lib() the `_lib` cache of the module that owns
it (op/_native/core.py; op/_native.py itself on a one-file tree) is replaced by a proxy that forwards each call and appends
    ["call", symbol, [args]]
to one list: integers and floats as they are; a pointer argument (by the entry point's argtypes) as "null", as its address
& 15 when it is an address (also one cast to a ctypes pointer), or as "host" for any other ctypes object (byref
out-parameters, host arrays).  An observer appends
    ["begin", name, info]  /  ["end"]
to the same list, the callable given as `latent_columns=` appends ["column", i] at each fetch, and a host query's answer
is kept as ["host", name, answer].  The last line printed names the bound fmgan_* symbols the run never called.  Needs a
GPU; uses nothing but the package (tools/ and tests/ helpers only for deterministic inputs).
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import torch  # noqa: E402

import synth  # noqa: E402
from op import _native  # noqa: E402

LOG = []


def _is_pointer(ctype):
    return ctype in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(ctype, type(ctypes.POINTER(ctypes.c_int)))


def _plain(arg, ctype):
    if not _is_pointer(ctype):
        return arg
    if isinstance(arg, ctypes.c_void_p):
        arg = arg.value
    elif isinstance(arg, ctypes._Pointer):          # an address cast to POINTER(c_int): the device slots of tiles_to_canvas
        arg = ctypes.cast(arg, ctypes.c_void_p).value
    if arg is None or arg == 0:
        return 'null'
    return arg & 15 if isinstance(arg, int) else 'host'


class RecordingLib:
    """Stands in for the ctypes library behind _native.lib(): same attributes, every call logged before it is made."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        argtypes = fn.argtypes

        def call(*args):
            LOG.append(['call', name, [_plain(a, t) for a, t in zip(args, argtypes)]])
            return fn(*args)
        setattr(self, name, call)
        return call


class RecordingObserver:
    wants_paths = False

    def begin(self, name, info):
        LOG.append(['begin', name, list(info)])
        return None

    def end(self, token):
        LOG.append(['end'])


def section(name):
    LOG.append(['section', name])
    torch.manual_seed(20)


def t(name, shape, d, **kw):
    return synth.tensor('record/' + name, shape, **kw).to(d)


def generator(d):
    import stylegan2
    G = stylegan2.Generator(64, 64, 2)
    G.load_state_dict(synth.state_dict('generator', G.state_dict(), seed=3))
    G = G.to(d)
    cin = G.conv1.conv.weight.shape[2]
    lat, tsr = t('lat', (2, G.n_latent, 64), d), t('tsr', (2, cin, 4, 4), d)
    kw = dict(input_is_latent=True, use_external_input_tensor=True, external_input_tensor=tsr)
    G.eval()
    with torch.no_grad():
        section('generator plain')
        G(None, latent_styles=[lat], **kw)
        section('generator return_rgb_list')
        G(None, latent_styles=[lat], return_rgb_list=True, **kw)
        section('generator comod')
        G(None, use_external_input_tensor=True, external_input_tensor=tsr,
          comod=(t('w', (2, 64), d), t('wplus', (1, G.n_latent, 64), d), None))
    G.train()
    section('generator backward')
    lat_g = lat.clone().requires_grad_(True)
    G(None, latent_styles=[lat_g], **kw).square().mean().backward()
    section('generator PPL_regularize')
    G.zero_grad(set_to_none=True)
    lat_g = lat.clone().requires_grad_(True)
    img, lengths = G(None, latent_styles=[lat_g], PPL_regularize=True, **kw)
    ((lengths - 0.5).pow(2).mean() + 0 * img[0, 0, 0, 0]).backward()


def _g(size, dim, d):
    """(G, W+ [2,n,dim], tensor [2,cin,4,4], W [2,dim], per-frame W+ [2,n,dim]) of a seeded Generator(size, dim, 2)."""
    import stylegan2
    G = stylegan2.Generator(size, dim, 2)
    G.load_state_dict(synth.state_dict('generator', G.state_dict(), seed=3))
    G = G.to(d).eval()
    n, cin = G.n_latent, G.conv1.conv.weight.shape[2]
    tag = f'g{size}/'
    return (G, t(tag + 'lat', (2, n, dim), d), t(tag + 'tsr', (2, cin, 4, 4), d), t(tag + 'w', (2, dim), d),
            t(tag + 'wplus', (2, n, dim), d, scale=0.5, shift=1.0))


def generator_styles(d):
    """Every way the Generator's layers get their style (W+ tensor, column callable, style bank, per-layer comod), with the
    column fetches in the log: for refactors of the host code between the launches."""
    import stylegan2
    G, lat, tsr, w, wplus = _g(64, 64, d)
    ext = dict(use_external_input_tensor=True, external_input_tensor=tsr)

    def column(i):
        LOG.append(['column', i])
        return lat[:, i]

    with torch.no_grad():
        section('generator latent_columns')
        G(None, latent_columns=column, **ext)
        section('generator comod sliced per-frame')
        G(None, comod=(w, wplus, [0, 3, 4]), **ext)
        prev = stylegan2.STYLE_BANK
        try:
            stylegan2.STYLE_BANK = False
            section('generator comod, STYLE_BANK off')
            G(None, comod=(w, wplus[:1].contiguous(), None), **ext)
            section('generator comod sliced per-frame, STYLE_BANK off')
            G(None, comod=(w, wplus, [0, 3, 4]), **ext)
        finally:
            stylegan2.STYLE_BANK = prev
        section('generator return_style_scalars')
        G(None, latent_styles=[lat], input_is_latent=True, return_style_scalars=True, **ext)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            section('generator plain under autocast')
            G(None, latent_styles=[lat], input_is_latent=True, **ext)
            section('generator comod under autocast')
            G(None, comod=(w, wplus, [0, 3, 4]), **ext)
        # the smallest Generator that reaches the Winograd form, the fused RGB epilogue and the row-march blur
        G, lat, tsr, w, wplus = _g(256, 512, d)
        ext = dict(use_external_input_tensor=True, external_input_tensor=tsr, randomize_noise=False)
        section('generator 256 plain')
        G(None, latent_styles=[lat], input_is_latent=True, **ext)
        section('generator 256 comod')
        G(None, comod=(w, wplus, [0, 3, 4]), **ext)


def small_ops(d):
    from op import upfirdn2d, fused_leaky_relu, face_region, lpips_distance, eval_scores
    section('upfirdn2d')
    x = t('ufd/x', (2, 3, 16, 16), d)
    k1 = torch.tensor([1., 3., 3., 1.])
    k = (k1[None, :] * k1[:, None] / k1.sum() ** 2).to(d)
    upfirdn2d(x, k * 4, up=2, pad=(2, 1))
    upfirdn2d(x, k, down=2, pad=(1, 1))
    upfirdn2d(x, k, pad=(2, 1))
    section('fused_leaky_relu')
    a, b = t('act/x', (2, 4, 16, 16), d).requires_grad_(True), t('act/b', (4,), d).requires_grad_(True)
    fused_leaky_relu(a, b).square().sum().backward()
    section('face_region')
    render, image = t('face/r', (2, 3, 32, 32), d, dist='uniform'), t('face/g', (2, 3, 32, 32), d).requires_grad_(True)
    render[:, :, :8] = -1.0
    face_region.face_region_loss(render, image).backward()
    _native.render_mask(render)
    section('lpips_distance')
    f0 = t('lpips/f0', (2, 64, 8, 8), d).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    f1 = t('lpips/f1', (2, 64, 8, 8), d).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    lpips_distance(f0, f1, t('lpips/w', (1, 64, 1, 1), d).abs()).sum().backward()
    section('encoder glue')
    with torch.no_grad():
        xe = t('glue/x', (2, 64, 8, 8), d).contiguous(memory_format=torch.channels_last)
        bn = (t('glue/m', (64,), d), t('glue/v', (64,), d).abs() + 0.5, t('glue/g', (64,), d), t('glue/b', (64,), d), 1e-5)
        _native.bn_prelu(xe, bn, t('glue/slope', (64,), d), want_y=True, bn_next=bn, sub_stride=2)
        partial = _native.se_pool(xe)
        gate = _native.se_gate(partial, 64, bn, t('glue/fc1', (16, 64, 1, 1), d), t('glue/fc2', (64, 16, 1, 1), d))
        _native.ir_tail(xe, bn, gate, xe, 1, None, bn)
    section('face_input')
    with torch.no_grad():
        eval_scores.face_input(t('fi/a', (2, 3, 128, 128), d, dist='uniform'), t('fi/b', (2, 3, 128, 128), d, dist='uniform'),
                               want_gray_b=True, want_l1=True)
    section('images')
    imgs = (t('img/u8', (2, 24, 20, 3), d, dist='uniform') * 127 + 128).clamp(0, 255).to(torch.uint8)
    _native.resize_images(imgs, 12, 10)
    _native.resize_images(imgs, 12, 10, to_tensor=True)
    _native.tensor_to_images(t('img/f32', (2, 3, 12, 10), d, dist='uniform'))
    from op.canvas import tiles_to_canvas
    canvas = torch.zeros((2, 9, 23, 3), dtype=torch.uint8, device=d)
    tiles_to_canvas(t('img/tiles', (3, 3, 12, 12), d, dist='uniform'), canvas, [(1, 2, 1), (0, 0, 8), (1, 1, 16)], 6)


def host(name, *args, **kw):
    """A host query of _native, with its answer in the log."""
    value = getattr(_native, name)(*args, **kw)
    LOG.append(['host', name, value.tolist() if torch.is_tensor(value) else value])
    return value


def _fir(d):
    k1 = torch.tensor([1., 3., 3., 1.])
    return (k1[None, :] * k1[:, None] / k1.sum() ** 2).to(d)


def activations(d):
    """csrc/act16.hip, fused_bias_act.hip and the fused blur of upfirdn2d.hip: tests/test_act16_gpu.py's [1, 2, 8, 8] and a
    [B, C] tensor (planes of one element: the hw < 64 branch of the 16-bit backward); tests/test_hip_ops.py's plane-tile
    row for the fused blur, and its 5 x 5 FIR, which the library declines."""
    from op import upfirdn2d, fused_leaky_relu
    k = _fir(d)

    def sixteen(dtype, tag):
        for shape in ((1, 2, 8, 8), (2, 3)):
            a = t(f'act16/{tag}/x{len(shape)}', shape, d).to(dtype).requires_grad_(True)
            b = t(f'act16/{tag}/b{len(shape)}', (shape[1],), d).requires_grad_(True)
            fused_leaky_relu(a, b).float().square().sum().backward()
        x = t(f'act16/{tag}/ufd', (1, 2, 8, 8), d).to(dtype)
        upfirdn2d(x, k, pad=(2, 1))
        upfirdn2d(x, k * 4, up=2, pad=(2, 1))

    section('16-bit activations, bf16')
    sixteen(torch.bfloat16, 'bf16')
    section('16-bit activations, f16 on the generic kernels')
    sixteen(torch.float16, 'f16')
    with _native.activation_io('16'):
        host('current_activation_io')
        section("16-bit activations under activation_io('16'), bf16")
        sixteen(torch.bfloat16, 'io/bf16')
        section("16-bit activations under activation_io('16'), f16")
        sixteen(torch.float16, 'io/f16')
    section('prelu_backward')
    _native.prelu_backward(t('prelu/x', (6, 8), d), t('prelu/g', (6, 8), d), t('prelu/slope', (8,), d))
    section('noise_bias_act, upfirdn2d_strided, blur_noise_bias_act')
    b, c, in_h, in_w, pad = 1, 2, 9, 63, (1, 1)
    nw, bias = t('blur/nw', (1,), d), t('blur/b', (c,), d)
    for taps in (4, 5):                                 # 4 x 4: the plane-tile kernel; 5 x 5: declined, the two-pass form
        kt = t(f'blur/k{taps}', (taps, taps), d)
        oh, ow = host('upfirdn2d_out_size', in_h, in_w, taps, taps, 1, 1, 1, 1, pad[0], pad[1], pad[0], pad[1])
        host('aligned_rows_shape', b, c, in_h, in_w, pad[0])
        buf, p0, ps, rs = _native.aligned_rows_buffer(b, c, in_h, in_w, pad[0], d)
        off = pad[0] % 4
        buf.zero_()
        buf[:, :, off:off + in_w] = t('blur/x', (b * c, in_h, in_w), d)
        nz = t(f'blur/n{taps}', (1, 1, oh, ow), d)
        serves = host('blur_noise_bias_act_serves', b, c, in_h, in_w, ps, rs, (taps, taps), pad)
        out = _native.blur_noise_bias_act(p0, d, b, c, in_h, in_w, ps, rs, kt, pad, nz, nw, bias, 0.2, 2 ** 0.5)
        assert (out is not None) == serves == (taps == 4)
        y = _native.upfirdn2d_strided(p0, d, b * c, in_h, in_w, ps, rs, kt, pad[0], pad[1], pad[0], pad[1])
        _native.noise_bias_act(y.view(b, c, oh, ow), nz, nw, bias, 0.2, 2 ** 0.5)


def convolutions(d):
    """The modconv family called directly: tests/test_hip_modconv_bf16.py's (1, 16, 32, 40, 33), tests/test_native_launch.py's
    Winograd case, tests/test_psp_heads_x3.py's (1, 8, 32, 2, 2), tests/test_hip_modconv.py's weight-gradient tables."""
    b, cin, cout, h, w = 1, 16, 32, 40, 33
    x, wgt = t('mc/x', (b, cin, h, w), d), t('mc/w', (cout, cin, 3, 3), d)
    s = t('mc/s', (b, cin), d, shift=1.0, scale=0.5)
    scale = 1.0 / (cin * 9) ** 0.5
    section('modconv_weight_prep, modconv_demod, modconv_wsq')
    wt = _native.modconv_weight_prep(wgt, scale)
    dm = _native.modconv_demod(wgt, s, scale)
    _native.modconv_demod(wgt, s, scale, wsq=_native.modconv_wsq(wgt))
    for precision in ('bf16', 'bf16x3'):
        section(f'modconv2d under {precision}')
        with _native.modconv_precision(precision):
            host('current_modconv_precision')
            _native.modconv2d(x, wt, s, dm, 0)
    section('winograd steps alone')
    b, c, h = 1, 8, 16
    x, wgt = t('wino/x', (b, c, h, h), d), t('wino/w', (c, c, 3, 3), d)
    s = t('wino/s', (b, c), d, shift=1.0, scale=0.5)
    scale = 1.0 / (c * 9) ** 0.5
    u = _native.wino_weight(_native.modconv_weight_prep(wgt, scale))
    v = _native.wino_input(x, s)
    _native.wino_output(torch.bmm(u, v), _native.modconv_demod(wgt, s, scale), b, h, h)
    section('conv3x3s2_bf16x3')
    b, cin, cout, h, w = 1, 8, 32, 2, 2
    host('conv3x3s2_bf16x3_supported', b, cin, cout, h, w)
    x, bias = t('x3/x', (b, cin, h, w), d), t('x3/b', (cout,), d)
    img = _native.conv_weight_to_bf16x3(t('x3/w', (cout, cin, 3, 3), d))
    assert _native.conv3x3s2_bf16x3(x, img, bias, cout, 0.01) is not None
    assert _native.conv3x3s2_bf16x3(x, img, bias, cout, 0.01, channels_last=True) is not None
    section('conv3x3_bf16x3')
    xcl = x.contiguous(memory_format=torch.channels_last)
    host('conv3x3_bf16x3_supported', b, cin, cout, h, w, 1, True)
    assert _native.conv3x3_bf16x3(xcl, img, cout, 1, 'prelu', bias, channels_last=True) is not None
    assert _native.conv3x3_bf16x3(xcl, img, cout, 2, None, channels_last=True) is not None
    assert _native.conv3x3_bf16x3(x, img, cout, 2, 'lrelu', bias, 0.01) is not None
    section('conv3x3_tail_bf16x3')        # tests/test_psp_tail_x3.py's 5-wide case
    b, cin, cout, h, w = 1, 16, 64, 10, 9
    host('conv3x3_tail_bf16x3_select', b, cin, cout, h, w)
    xcl, bias = t('tail/x', (b, cin, h, w), d).contiguous(memory_format=torch.channels_last), t('tail/b', (cout,), d)
    img = _native.conv_weight_to_bf16x3(t('tail/w', (cout, cin, 3, 3), d), 'conv_tail_weight_bf16x3')
    assert _native.conv3x3_tail_bf16x3(xcl, img, bias, cout, 0.01) is not None
    assert _native.conv3x3_tail_bf16x3(xcl, img, bias, cout, 0.01, channels_last=False) is not None
    section('torgb_backward')
    b, cin, hw = 2, 8, 4
    _native.torgb_backward(t('rgb/x', (b, cin, hw, hw), d), t('rgb/go', (b, 3, hw, hw), d), t('rgb/w', (1, 3, cin, 1, 1), d),
                           t('rgb/s', (b, cin), d, shift=1.0, scale=0.5), 1.0 / cin ** 0.5)
    section('modconv_wgrad')
    # (mode, b, cin, cout, h, w): the 64 x 64-tile and the 32 x 32-tile kernel of the plain conv, the transposed, the stride-2
    for mode, b, cin, cout, h, w in ((0, 1, 48, 200, 9, 16), (0, 1, 32, 32, 128, 128), (1, 2, 64, 64, 16, 16),
                                     (2, 2, 64, 96, 35, 35)):
        oh, ow = (2 * h + 1, 2 * w + 1) if mode == 1 else (((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == 2 else (h, w))
        tag = f'wg/{mode}/{cin}'
        go, x = t(tag + '/go', (b, cout, oh, ow), d), t(tag + '/x', (b, cin, h, w), d)
        s, dmod = t(tag + '/s', (b, cin), d, shift=1.0, scale=0.5), t(tag + '/d', (b, cout), d, shift=1.0, scale=0.3)
        assert _native.modconv_wgrad(go, dmod, x, s, 0.37, mode=mode) is not None
        assert (_native.modconv_wgrad(go, dmod, x, s, 0.37, fast_only=True, mode=mode) is None) == (cin < 48)
    section('modconv host queries')
    host('modconv2d_select', 8, 32, 32, 64, 64, 0)
    host('modconv2d_select', 8, 32, 32, 1024, 1024, 0, rgb=True)
    host('modconv2d_rgb_fusable', 8, 32, 32, 1024, 1024)
    host('modconv2d_tiles')
    host('modconv_wgrad_select', 1, 48, 200, 9, 16, 0)
    host('modconv_wgrad_select', 2, 64, 64, 16, 16, 1, aligned16=False)
    host('wino_select', 'input', 8, 512, 16, 16)
    host('wino_select', 'output', 8, 512, 16, 16)
    host('wino_select', 'output', 8, 256, 128, 128)


def live_weights(d):
    from op.live_weights import LiveWeights
    G = _g(64, 64, d)[0]
    section('LiveWeights refresh')
    assert LiveWeights(G).refresh()


def _u8(name, shape, d):
    return (t(name, shape, d, dist='uniform') * 127 + 128).clamp(0, 255).to(torch.uint8)


def images(d):
    """csrc/image_io.hip, resize_plan.cpp, image_bank.hip: tests/test_dataset_gpu.py's 8 x 8 banks and its PAIR triple."""
    section('images_to_tensor, bank_gather')
    _native.images_to_tensor(_u8('img/u8', (2, 24, 20, 3), d))
    host('resize_output_size', 24, 20, 12)
    host('resize_plan', 24, 20, 12, 10)
    banks = [_u8(f'bank/{k}', (21, 8, 8, 3), d) for k in 'ab']
    index = torch.tensor([5, 20, 0, 9, 9, 1, 17, 3], dtype=torch.int32, device=d)
    _native.bank_gather(banks, index, None, 0, 8, 1, [(0, 0, 0, 1, 0), (1, 0, 1, 1, 0), (0, 0, 1, 1, 0)])


def stages(d):
    """The loss and evaluation stages: tests/ppl_cases.py (g64), projection_cases.py (c256_mse_mask), fid_cases.py (d64),
    landmark_cases.py (crop_small, the distance case, a decode case's shape)."""
    from op import landmark
    from op.fid_stats import Feature_Statistics
    shift, scale = t('stage/shift', (1, 3, 1, 1), d, scale=0.1), t('stage/scale', (1, 3, 1, 1), d, scale=0.1, shift=0.5)
    section('lpips_pair_input')
    assert _native.lpips_pair_input(t('ppl/img', (2, 3, 64, 64), d), shift, scale, (0, 0, 64, 64), 1) is not None
    section('projection_loss')
    x, target = t('proj/x', (1, 3, 256, 256), d), t('proj/target', (1, 3, 256, 256), d, dist='uniform')
    mask = (t('proj/mask', (256, 256), d, dist='uniform') + 1) / 2
    partial, y = _native.projection_loss_fwd(x, target, mask, shift, scale)
    g_y = t('proj/gy', (1, 3, 256, 256), d).contiguous(memory_format=torch.channels_last)
    assert _native.projection_loss_bwd(x, target, mask, g_y, t('proj/k', (1,), d), scale) is not None
    section('fid_stats')
    host('fid_stats_serves', 200, 64)
    stats = Feature_Statistics(64, d, shift=t('fid/shift', (64,), d))
    stats.update(t('fid/feat', (200, 64), d))
    stats.finish()
    section('inception_input')
    assert _native.inception_input(t('fid/img', (1, 3, 256, 256), d, dist='uniform'), True) is not None
    section('landmark')
    host('face_input_pool', 256)
    host('face_crop_serves', 3, 48, 40, 32)
    img = t('lm/img', (3, 3, 48, 40), d, dist='uniform').requires_grad_(True)
    boxes = [(9, 14, 31, 35), (-6, -1, 47, 52), (-23, -28, 77, 72)]
    landmark.face_crop(img, boxes, r=32, fuse=True).square().sum().backward()
    assert landmark.detector_input(img.detach(), fuse=True) is not None
    host('heatmap_distance_serves', 3, 4 * 64 * 64)
    a = t('lm/a', (3, 4, 64, 64), d, scale=0.3).requires_grad_(True)
    b = t('lm/b', (3, 4, 64, 64), d, scale=0.3).requires_grad_(True)
    landmark.heatmap_distance(a, b, fuse=True).sum().backward()
    landmark.landmark_decode(t('lm/hm', (2, 5, 64, 64), d), t('lm/center', (2, 2), d, shift=128.0),
                             t('lm/scale', (2,), d, shift=2.0, scale=0.1), fuse=True)


def optimisers(d):
    """csrc/lbfgs.hip through op.lbfgs.FusedState on tests/lbfgs_cases.py's four tensors; csrc/train_loop.hip through
    op.ema.EmaPlan and on a ledger row as tests/test_train_loop_gpu.py writes one."""
    from op.ema import EmaPlan
    from op.lbfgs import FusedState
    shapes = ((2, 3, 8), (1, 1, 4, 4), (1, 1, 4, 4), (1, 1, 8, 8))
    params = [t(f'lbfgs/p{k}', shape, d) for k, shape in enumerate(shapes)]
    for k, p in enumerate(params):
        p.grad = t(f'lbfgs/g{k}', p.shape, d)
    state = FusedState(params, 3)
    section('lbfgs')
    state.direction(1.0, 1e-10, False)
    state.update(0.5)
    state.gather()
    for k, p in enumerate(params):
        p.grad = t(f'lbfgs/h{k}', p.shape, d)
    state.direction(0.5, 1e-10, True)
    section('ema, loss_row')
    host('ema_blocks', 5000)
    ema, net = torch.nn.Linear(8, 4).to(d), torch.nn.Linear(8, 4).to(d)
    for m, tag in ((ema, 'ema'), (net, 'net')):
        m.load_state_dict({k: t(f'ema/{tag}/{k}', v.shape, d) for k, v in m.state_dict().items()})
    EmaPlan(ema, net).update(0.999)
    ring = torch.zeros((3, 16), dtype=torch.float32, device=d)
    store = t('row/store', (8,), d)
    _native.loss_row([store[3], None, t('row/v', (1,), d)], ring[1])
    try:                                                # refused on the host: the status text is asked of the library
        _native.loss_row([None] * 17, ring[0])
    except RuntimeError as e:
        LOG.append(['host', 'loss_row refusal', str(e)])


def never_called(real):
    """Bound fmgan_* symbols (those lib() gave a signature) that the run did not call, sorted."""
    bound = {n for n, fn in vars(real).items() if n.startswith('fmgan_') and fn.argtypes is not None}
    return sorted(bound - {e[1] for e in LOG if e[0] == 'call'})


def main():
    out = sys.argv[1]
    d = torch.device('cuda', 0)
    real = _native.lib()
    owner = getattr(_native, 'core', _native)           # the module that owns `_lib`: op/_native/core.py, or the one file
    owner._lib = RecordingLib(real)
    _native.set_observer(RecordingObserver())
    try:
        generator(d)
        generator_styles(d)
        small_ops(d)
        activations(d)
        convolutions(d)
        live_weights(d)
        images(d)
        stages(d)
        optimisers(d)
        torch.cuda.synchronize()
    finally:
        _native.set_observer(None)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(LOG, f, indent=0, default=repr)
    calls = [e[1] for e in LOG if e[0] == 'call']
    print(json.dumps(dict(out=out, calls=len(calls), events=sum(1 for e in LOG if e[0] == 'begin'),
                          entry_points=len(set(calls)), host=sum(1 for e in LOG if e[0] == 'host'))))
    print('never called: ' + ' '.join(never_called(real)))


if __name__ == '__main__':
    main()
