#!/usr/bin/env python3
"""Record every call into libfmgan_hip.so and every observer event of a fixed, seeded workload, as JSON.

    python tools/record_native_calls.py OUT.json

For refactors of op/_native.py: run it on the commit before and on the commit after and compare the two files — the same
entry points with the same arguments in the same order, bracketed by the same (name, info) events, is the same work on the
GPU.  After the first _native.lib() the module's `_lib` cache is replaced by a proxy that forwards each call and appends
    ["call", symbol, [args]]
to one list: integers and floats as they are; a pointer argument (by the entry point's argtypes) as "null", as its address
& 15 when it is an address (also one cast to a ctypes pointer), or as "host" for any other ctypes object (byref
out-parameters, host arrays).  An observer appends
    ["begin", name, info]  /  ["end"]
to the same list, and the callable given as `latent_columns=` appends ["column", i] at each fetch.  Needs a GPU; uses nothing but the package (tools/ and tests/ helpers only for deterministic inputs).
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


def main():
    out = sys.argv[1]
    d = torch.device('cuda', 0)
    _native.lib()
    _native._lib = RecordingLib(_native._lib)
    _native.set_observer(RecordingObserver())
    try:
        generator(d)
        generator_styles(d)
        small_ops(d)
        torch.cuda.synchronize()
    finally:
        _native.set_observer(None)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(LOG, f, indent=0, default=repr)
    calls = sum(1 for e in LOG if e[0] == 'call')
    print(json.dumps(dict(out=out, calls=calls, events=sum(1 for e in LOG if e[0] == 'begin'))))


if __name__ == '__main__':
    main()
