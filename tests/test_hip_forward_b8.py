"""The headline configuration — batch 8, Generator(1024, 512, 8) — held to references of its own.

Kernel dispatch depends on the batch (stylegan2.winograd_pays, the tile table of csrc/modconv_fwd.hip, the placement
workspaces of op/placement.py, the fused ToRGB of the last resolution), and the other Generator tests run at B = 1 or 2.

Part 1, per layer: every synthesis layer of the B = 8 forward, RUN AS A MODULE (StyledConv.forward / fused_with_rgb / ToRGB
under no_grad, so the dispatch is part of what is tested), against the fp32 oracle (oracle/torch_oracle.py, the reference's
weight-modulated grouped convolution) and a float64 evaluation of the same operator (input-modulated, one convolution for
the batch — as test_bf16x3_kernel_has_fp32_accuracy builds it — then the oracle's blur and epilogue in float64).
Layers up to 128^2: the whole tensor.  Larger layers: windows on zero-filled input crops (tests/parity.py).
Gates, the project's own: parity.tol (2e-5 of max|ref|, rtol 1e-5) against the fp32 oracle, and
|HIP - fp64| <= 4 |oracle fp32 - fp64| + 2e-6 max|fp64|.  A launch observer asserts that the path that ran is the path meant.

Part 2, end to end: tests/golden/generator_b8.npz (tools/make_golden.py gen_generator_b8: the reference at B = 8, every image
of the RGB pyramid, fp32 and float64) against the default forward (placement workspaces, fused last ToRGB), the
return_rgb_list forward, and the forward with the Winograd form switched off.

Every figure is printed before it is asserted (pytest -s): profiles/parity_b8_layers.md is a copy of one such run."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import launches
import synth
from gpumem import dev
from nets import load
from parity import crop, img_close, input_window, ref_errors, tol, within_reference

pytestmark = pytest.mark.gpu

B = 8
WINDOW = 32
SAMPLES = [0, 3, 7]          # of the windows of the large layers: first, a middle and the last sample of the batch


# ------------------------------------------------------------------------------------------------------- layer table
def _layer_table():
    """The synthesis layers of stylegan2.Generator(1024, 512, 8) in forward order, read off the module itself (built on
    the meta device: shapes only).  kind: 'plain' / 'up' StyledConv, 'rgb' ToRGB; res = output resolution."""
    import stylegan2
    with torch.device('meta'):
        g = stylegan2.Generator(1024, 512, 8)
    rows = [dict(name='conv1', kind='plain', cin=g.conv1.conv.in_channel, cout=g.conv1.conv.out_channel, res=4),
            dict(name='to_rgb1', kind='rgb', cin=g.to_rgb1.conv.in_channel, cout=3, res=4)]
    res = 4
    for j, to_rgb in enumerate(g.to_rgbs):
        up, plain = g.convs[2 * j], g.convs[2 * j + 1]
        assert up.conv.upsample and not plain.conv.upsample
        res *= 2
        rows.append(dict(name=f'convs.{2 * j}', kind='up', cin=up.conv.in_channel, cout=up.conv.out_channel, res=res))
        rows.append(dict(name=f'convs.{2 * j + 1}', kind='plain', cin=plain.conv.in_channel, cout=plain.conv.out_channel,
                         res=res))
        rows.append(dict(name=f'to_rgbs.{j}', kind='rgb', cin=to_rgb.conv.in_channel, cout=3, res=res))
    assert res == 1024 and len(rows) == 2 + 3 * 8
    return rows


LAYERS = _layer_table()
STYLED = [r for r in LAYERS if r['kind'] != 'rgb']
TORGB = [r for r in LAYERS if r['kind'] == 'rgb']


def _in_res(r):
    return r['res'] // 2 if r['kind'] == 'up' else r['res']


def _x3_supported(r):
    from op import _native
    return bool(_native.lib().fmgan_modconv2d_bf16x3_supported(B, r['cin'], r['cout'], _in_res(r), _in_res(r),
                                                               1 if r['kind'] == 'up' else 0))


def _lid(r):
    return f"{r['name']}_{r['kind']}_{r['cin']}to{r['cout']}_at{r['res']}"


STYLED_PARAMS = [pytest.param(r, p, id=f'{_lid(r)}-{p}') for r in STYLED for p in ('f32', 'bf16x3')
                 if p == 'f32' or _x3_supported(r)]


def _winograd_layer(r):
    """The four layers stylegan2.winograd_pays names at B = 8."""
    return r['kind'] == 'plain' and (r['cin'], r['cout'], r['res']) in ((512, 512, 16), (512, 512, 32), (512, 512, 64),
                                                                        (256, 256, 128))


def _windows(res):
    """(windows (y0, x0, h, w), samples).  Up to 128^2: the whole tensor, every sample.  Above: 32 x 32 windows at even
    origins — the four corners, the last rows in the interior of the width and the last columns in the interior of the
    height, an interior window off every power-of-two grid, and one window centred on (res/2, res/2).  res/2 is a multiple
    of 128 here, so that window crosses in BOTH directions a boundary of every tiling in play: the plain conv's 128- and
    256-position tiles (32 wide x 4 or 8 tall, csrc/modconv_fwd.hip plan_segment / pick_tw_log2), the transposed conv's tiles
    (32 x 4 positions of one output phase = 64 x 8 output pixels), the bf16x3 kernel's tiles and the fused blur's
    64-column wave strips."""
    if res <= 128:
        return [(0, 0, res, res)], list(range(B))
    e, mid, c = res - WINDOW, (res // 3) & ~1, res // 2 - WINDOW // 2
    wins = [(0, 0), (0, e), (e, 0), (e, e), (e, mid), (mid, e), (mid, mid + 2), (c, c)]
    return [(y0, x0, WINDOW, WINDOW) for y0, x0 in wins], SAMPLES


# ------------------------------------------------------------------------------------------------------- fixtures, caches
@pytest.fixture(scope='module')
def gen():
    import stylegan2
    g = load(stylegan2.Generator(1024, 512, 8), 'generator', 4)
    yield g
    del g
    _CACHE.clear()
    torch.cuda.empty_cache()


_CACHE = {}        # inputs and references of the layer under test (one layer at a time: a 1024^2 input is 1 GB)


def _cached(layer, key, make):
    if _CACHE.get('layer') != layer:
        _CACHE.clear()
        _CACHE['layer'] = layer
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _module(g, r):
    m = g
    for part in r['name'].split('.'):
        m = m[int(part)] if part.isdigit() else getattr(m, part)
    return m


def _cpu_sd(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def _observe():
    """The launches of the block; wants_paths makes _native note the fused blur's kernel id."""
    return launches.observed(wants_paths=True)


# ------------------------------------------------------------------------------------------------------- references
def _core32(sd, xc, lat, up, demod):
    """fp32 oracle: ModulatedConv2d as the reference states it (+ the blur of the upsampling branch)."""
    from oracle import torch_oracle as T
    return T.modulated_conv2d(xc, lat, sd['conv.weight'], sd['conv.modulation.weight'], sd['conv.modulation.bias'],
                              demodulate=demod, upsample=up, blur_kernel=[1, 3, 3, 1])


def _core64(sd, xc, lat, up, demod):
    """float64, input-modulated: out = demod * conv(scale W, s * x), then the oracle's upfirdn2d for the blur."""
    from oracle import torch_oracle as T
    w = sd['conv.weight'][0].double()
    cin = w.shape[1]
    s = T.equal_linear(lat.double(), sd['conv.modulation.weight'].double(), sd['conv.modulation.bias'].double())
    wq = w * (1 / math.sqrt(cin * 9))
    u = xc.double() * s[:, :, None, None]
    y = F.conv_transpose2d(u, wq.transpose(0, 1), stride=2) if up else F.conv2d(u, wq, padding=1)
    if demod:
        y = y * torch.rsqrt((s * s) @ (wq * wq).sum((2, 3)).t() + 1e-8)[:, :, None, None]
    if up:
        y = T.upfirdn2d(y, T.make_kernel([1, 3, 3, 1]).double() * 4, pad=(1, 1))
    return y


def _cores(r, sd, x, lat, demod=True):
    """[(window, samples, core32, core64)] of a StyledConv: the convolution (+ demodulation, + blur) before the epilogue."""
    up = r['kind'] == 'up'
    wins, samples = _windows(r['res'])
    out = []
    with torch.no_grad():
        for (y0, x0, wh, ww) in wins:
            iy0, ix0, ih, iw, oy, ox = input_window(1 if up else 0, y0, x0, wh, ww, blur=up)
            xc = crop(x, iy0, ix0, ih, iw)[samples]
            c32 = _core32(sd, xc, lat[samples], up, demod)[:, :, oy:oy + wh, ox:ox + ww]
            c64 = _core64(sd, xc, lat[samples], up, demod)[:, :, oy:oy + wh, ox:ox + ww]
            assert c32.shape[2:] == (wh, ww) and c64.shape == c32.shape
            out.append(((y0, x0, wh, ww), samples, c32.contiguous(), c64.contiguous()))
    return out


def _epilogue(core, sd, noise, win, samples):
    """NoiseInjection + FusedLeakyReLU of the oracle in core's dtype; noise [B or 1, 1, H, W]."""
    from oracle import torch_oracle as T
    y0, x0, wh, ww = win
    nz = noise[:, :, y0:y0 + wh, x0:x0 + ww]
    nz = nz[samples] if nz.shape[0] != 1 else nz
    out = core + sd['noise.weight'].to(core.dtype) * nz.to(core.dtype)
    return T.fused_leaky_relu(out, sd['activate.bias'].to(core.dtype))


def _gates(tag, got, refs):
    """Both gates on every window; prints the figures first.  got: device tensor [B,C,H,W]; refs: [(win, samples, r32, r64)]."""
    worst = (0.0, 0.0, 0.0)
    fails = []
    for (y0, x0, wh, ww), samples, r32, r64 in refs:
        a = got[:, :, y0:y0 + wh, x0:x0 + ww][samples].cpu().numpy()
        r32, r64 = r32.numpy(), r64.numpy()
        assert a.shape == r32.shape, (a.shape, r32.shape)
        e_hip, e_ref = ref_errors(a, r32, r64)
        d32 = float(np.abs(a - r32).max()) / max(1.0, float(np.abs(r32).max()))
        worst = tuple(max(p, q) for p, q in zip(worst, (e_hip, e_ref, d32)))
        t = tol(r32)
        if not np.all(np.abs(a - r32) <= t['atol'] + t['rtol'] * np.abs(r32)):
            fails.append(f'{tag} window {(y0, x0)}: |HIP - oracle fp32| = {d32:.3e} of max(1, max|ref|) exceeds 2e-5 / rtol 1e-5')
        if not within_reference(e_hip, e_ref):
            fails.append(f'{tag} window {(y0, x0)}: |HIP - fp64| = {e_hip:.3e} > 4 x {e_ref:.3e} + 2e-6')
    print(f'PARITY {tag}: |HIP-fp64| {worst[0]:.3e}  |oracle32-fp64| {worst[1]:.3e}  |HIP-oracle32| {worst[2]:.3e}', flush=True)
    assert not fails, '\n'.join(fails)


def _inputs(r):
    h = _in_res(r)
    x = _cached(r['name'], 'x', lambda: synth.tensor(f"b8/x/{r['cin']}x{h}", (B, r['cin'], h, h)))
    lat = synth.tensor(f"b8/{r['name']}/lat", (B, 512))
    noise = _cached(r['name'], 'noise', lambda: synth.tensor(f"b8/{r['name']}/noise", (B, 1, r['res'], r['res'])))
    return x, lat, noise


# ------------------------------------------------------------------------------------------------------- part 1: StyledConv
def test_layer_table_is_the_headline_forward():
    """17 StyledConvs and 9 ToRGBs; the Winograd rule names exactly four of them at B = 8; the fused ToRGB exists for the
    plain layers of the last three resolutions."""
    import stylegan2
    from op import _native
    assert len(STYLED) == 17 and len(TORGB) == 9
    assert [r['res'] for r in TORGB] == [4, 8, 16, 32, 64, 128, 256, 512, 1024]
    wino = [r for r in STYLED if r['kind'] == 'plain' and stylegan2.winograd_pays(B, r['cin'], r['cout'], r['res'], r['res'])]
    assert wino == [r for r in STYLED if _winograd_layer(r)] and len(wino) == 4
    fus = [r['res'] for r in STYLED if r['kind'] == 'plain' and _native.modconv2d_rgb_fusable(B, r['cin'], r['cout'], r['res'],
                                                                                             r['res'])]
    assert fus == [256, 512, 1024]


@pytest.mark.parametrize('r,precision', STYLED_PARAMS)
def test_styled_conv_at_batch_8(r, precision, gen):
    from op import _native
    d = dev()
    mod = _module(gen, r)
    conv = mod.conv
    assert (conv.in_channel, conv.out_channel, conv.upsample) == (r['cin'], r['cout'], r['kind'] == 'up')
    sd = _cpu_sd(mod)
    x, lat, noise = _inputs(r)
    cores = _cached(r['name'], 'cores', lambda: _cores(r, sd, x, lat))
    refs = [(w, s, _epilogue(c32, sd, noise, w, s), _epilogue(c64, sd, noise, w, s)) for w, s, c32, c64 in cores]
    xd, latd, nzd = x.to(d), lat.to(d), noise.to(d)
    h, res = _in_res(r), r['res']
    wino = precision == 'f32' and _winograd_layer(r)
    tag = f'{_lid(r)} {precision}'
    with torch.no_grad(), _native.modconv_precision(precision):
        with _observe() as rec:
            y = mod(xd, latd, noise=nzd)
        assert y.shape == (B, r['cout'], res, res)
        _gates(tag + (' winograd' if wino else ' module'), y, refs)
        # ---- the path that ran is the path meant (after the values: a wrong path with right values shows as such)
        contraction = 'modconv2d_bf16x3' if precision == 'bf16x3' else 'modconv2d'
        if r['kind'] == 'up':
            assert rec.seen[0] == (contraction, (B, r['cin'], r['cout'], h, h, 1)), rec.seen
            assert rec.names == [contraction, 'upfirdn2d'], rec.names          # one fused blur, no two-pass fall-back
            path = _native.BLUR_PATHS.get((B * r['cout'], 2 * h + 1, 2 * h + 1))
            # plane-tile below 64 columns, register row-march from 64, LDS-DMA ring from 256 (csrc/upfirdn2d.hip)
            assert path == (2 if res < 64 else (1 if res < 256 else 5)), (path, res)
        elif wino:
            assert rec.seen == [('modconv2d_winograd', (B, r['cin'], r['cout'], h, h, 0))], rec.seen
        else:
            assert rec.seen == [(contraction, (B, r['cin'], r['cout'], h, h, 0))], rec.seen

        if wino:
            assert torch.equal(mod(xd, latd, noise=nzd), y)                        # two calls, the same bits
            # the direct kernel on the same arguments (what FMGAN_NO_WINOGRAD=1 runs)
            s = conv.styles(latd)
            dm = _native.modconv_demod(conv.weight, s, conv.scale, conv.eps)
            kw = dict(noise_weight=mod.noise.weight, bias=mod.activate.bias, fuse_act=True,
                      alpha=mod.activate.negative_slope, act_scale=mod.activate.scale)
            with _observe() as rec:
                yd = _native.modconv2d(xd, conv.mfma_weight(), s, dm, 0, noise=nzd, **kw)
            assert rec.names == ['modconv2d']
            _gates(tag + ' direct', yd, refs)
            del yd
            # one noise plane for the whole batch
            refs1 = [(w, sm, _epilogue(c32, sd, noise[:1], w, sm), _epilogue(c64, sd, noise[:1], w, sm))
                     for w, sm, c32, c64 in cores]
            with _observe() as rec:
                y1 = mod(xd, latd, noise=nzd[:1].contiguous())
            assert rec.names == ['modconv2d_winograd']
            _gates(tag + ' winograd shared-noise', y1, refs1)
            del y1, refs1
            # no demodulation
            cores_nd = _cores(r, sd, x, lat, demod=False)
            refs_nd = [(w, sm, _epilogue(c32, sd, noise, w, sm), _epilogue(c64, sd, noise, w, sm)) for w, sm, c32, c64 in cores_nd]
            conv.demodulate = False
            try:
                with _observe() as rec:
                    ynd = mod(xd, latd, noise=nzd)
            finally:
                conv.demodulate = True
            assert rec.names == ['modconv2d_winograd']
            _gates(tag + ' winograd no-demod', ynd, refs_nd)
            del ynd, refs_nd, cores_nd

        # ---- the following ToRGB in the conv's epilogue, wherever the layer offers it at B = 8
        if r['kind'] == 'plain' and mod.rgb_fusable((B, 0, res, res), xd):
            assert precision == 'f32' and res in (256, 512, 1024)
            from oracle import torch_oracle as T
            to_rgb = _module(gen, dict(name=f"to_rgbs.{int(r['name'].split('.')[1]) // 2}"))
            assert to_rgb.conv.in_channel == r['cout']
            sd_rgb = {'R.' + k: v for k, v in _cpu_sd(to_rgb).items()}
            rgb_lat = synth.tensor(f"b8/{r['name']}/rgb_lat", (B, 512))
            skip_up = synth.tensor(f"b8/{r['name']}/skip_up", (B, 3, res, res))
            rgb_refs = []
            for (w, sm, a32, a64) in refs:
                y0, x0, wh, ww = w
                sk = skip_up[:, :, y0:y0 + wh, x0:x0 + ww][sm]
                rgb_refs.append((w, sm, T.to_rgb(sd_rgb, 'R', a32, rgb_lat[sm]) + sk,
                                 T.to_rgb({k: v.double() for k, v in sd_rgb.items()}, 'R', a64, rgb_lat[sm].double()) + sk.double()))
            for keep in (True, False):                       # keep_out=False is what the Generator asks for
                with _observe() as rec:
                    act, rgb = mod.fused_with_rgb(xd, latd, nzd, to_rgb, rgb_lat.to(d), skip_up.to(d), keep_out=keep)
                assert rec.seen == [('modconv2d', (B, r['cin'], r['cout'], res, res, 0))], rec.seen
                assert (act is not None) == keep and rgb.shape == (B, 3, res, res)
                if keep:
                    _gates(tag + ' fused-rgb activation', act, refs)
                _gates(tag + f' fused-rgb image keep_out={keep}', rgb, rgb_refs)
                del act, rgb
    del y, xd, nzd
    torch.cuda.empty_cache()


@pytest.mark.parametrize('r', TORGB, ids=_lid)
def test_to_rgb_at_batch_8(r, gen):
    """ToRGB as a module (1x1 modulated conv + bias + the upsampled skip of the previous resolution) against the oracle's
    to_rgb in fp32 and in float64; windows of the large layers take the skip crop that the 4-tap upsample reads."""
    from oracle import torch_oracle as T
    d = dev()
    mod = _module(gen, r)
    sd = {'R.' + k: v for k, v in _cpu_sd(mod).items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    res = r['res']
    x, lat, _ = _inputs(r)
    skip = synth.tensor(f"b8/{r['name']}/skip", (B, 3, res // 2, res // 2)) if res > 4 else None
    wins, samples = _windows(res)
    refs = []
    with torch.no_grad():
        for (y0, x0, wh, ww) in wins:
            xc = x[:, :, y0:y0 + wh, x0:x0 + ww][samples]
            r32 = T.to_rgb(sd, 'R', xc, lat[samples])
            r64 = T.to_rgb(sd64, 'R', xc.double(), lat[samples].double())
            if skip is not None:
                iy0, ix0, ih, iw, oy, ox = input_window(1, y0, x0, wh, ww, blur=True)
                sc = crop(skip, iy0, ix0, ih, iw)[samples]
                k4 = T.make_kernel([1, 3, 3, 1]) * 4
                r32 = r32 + T.upfirdn2d(sc, k4, up=2, pad=(2, 1))[:, :, oy:oy + wh, ox:ox + ww]
                r64 = r64 + T.upfirdn2d(sc.double(), k4.double(), up=2, pad=(2, 1))[:, :, oy:oy + wh, ox:ox + ww]
            refs.append(((y0, x0, wh, ww), samples, r32, r64))
        with _observe() as rec:
            y = mod(x.to(d), lat.to(d), None if skip is None else skip.to(d))
    assert rec.names.count('torgb') == 1 and rec.names.count('upfirdn2d') == (0 if skip is None else 1), rec.names
    _gates(_lid(r), y, refs)
    del y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------- part 2: end to end
def _b8_inputs(g):
    c = cases.GENERATOR_B8_CASE
    lat = synth.tensor(c['name'] + '/latent', (c['b'], g.n_latent, 512)).to(dev())
    tsr = synth.tensor(c['name'] + '/tsr', (c['b'], 512, 4, 4)).to(dev())
    return dict(latent_styles=[lat], input_is_latent=True, use_external_input_tensor=True, external_input_tensor=tsr,
                randomize_noise=False)


def _count_rgb_fusions(monkeypatch):
    """The fused conv + ToRGB entry reports to the observer under the plain conv's name: count its calls at the binding."""
    from op import _native
    calls = []
    orig = _native.modconv2d_rgb

    def counted(x, *a, **kw):
        calls.append(tuple(x.shape))
        return orig(x, *a, **kw)

    monkeypatch.setattr(_native, 'modconv2d_rgb', counted)
    return calls


def _image_gates(img, golden, i):
    g = golden('generator_b8')
    key = f"{cases.GENERATOR_B8_CASE['name']}/rgb{i}"
    a = img.detach().float().cpu().numpy()
    e_hip, e_ref = ref_errors(a[..., ::cases.b8_stride(a.shape[-1]), ::cases.b8_stride(a.shape[-1])], g[key + '/sub'],
                              g[key + '/sub64'])
    print(f'PARITY {key} {a.shape[-1]}^2: |HIP-fp64| {e_hip:.3e}  |reference32-fp64| {e_ref:.3e}', flush=True)
    img_close(a, g[key + '/sub'], g[key + '/stats'], cases.b8_stride(a.shape[-1]), g[key + '/sub64'])


def test_generator_b8_default_forward_vs_reference(gen, golden, monkeypatch):
    """The benchmark's forward: placement workspaces selected on the first call and reused on the second, the four Winograd
    layers, the last ToRGB in the 1024^2 conv's epilogue — against the reference's B = 8 image."""
    from op import _native, placement
    monkeypatch.setattr(placement, 'ENABLED', True)
    placement.forget()
    fusions = _count_rgb_fusions(monkeypatch)
    kw = _b8_inputs(gen)
    runs, seen = [], []
    with torch.no_grad():
        for _ in range(2):
            del fusions[:]
            with _observe() as rec:
                runs.append(gen(None, **kw))
            seen.append((rec.names.count('modconv2d_winograd'), list(fusions)))
    _image_gates(runs[0], golden, 8)
    assert torch.equal(runs[0], runs[1])
    assert seen == [(4, [(B, 32, 1024, 1024)])] * 2, seen
    # workspaces for exactly the upsampling layers whose intermediate reaches MIN_BYTES (256^2 -> 512^2, 512^2 -> 1024^2)
    want = set()
    for r in STYLED:
        if r['kind'] == 'up':
            shape = _native.aligned_rows_shape(B, r['cout'], r['res'] + 1, r['res'] + 1, 1)[0]
            if 4 * shape[0] * shape[1] * shape[2] >= placement.MIN_BYTES:
                want.add(r['name'])
    have = {r['name'] for r in STYLED if _module(gen, r) in placement._STORE}
    assert have == want == {'convs.12', 'convs.14'}, (have, want)
    assert len(placement._STORE) == 2
    placement.forget()


def test_generator_b8_rgb_pyramid_vs_reference(gen, golden, monkeypatch):
    """return_rgb_list=True keeps every ToRGB a kernel of its own: every image of the pyramid through the image gates, in
    order, so a failure names the first resolution that is off."""
    from op import placement
    fusions = _count_rgb_fusions(monkeypatch)
    with torch.no_grad(), _observe() as rec:
        rgbs = gen(None, return_rgb_list=True, **_b8_inputs(gen))
    assert len(rgbs) == 9
    for i, img in enumerate(rgbs):
        assert img.shape == (B, 3, 4 << i, 4 << i)
        _image_gates(img, golden, i)
    assert not fusions
    assert rec.names.count('modconv2d_winograd') == 4 and rec.names.count('torgb') == 9, rec.names
    placement.forget()


def test_generator_b8_direct_kernels_vs_reference(gen, golden, monkeypatch):
    """The default forward with the Winograd form switched off: the direct MFMA kernel on all 17 layers at B = 8."""
    import stylegan2
    from op import placement
    monkeypatch.setattr(stylegan2, 'WINOGRAD', False)
    fusions = _count_rgb_fusions(monkeypatch)
    with torch.no_grad(), _observe() as rec:
        img = gen(None, **_b8_inputs(gen))
    _image_gates(img, golden, 8)
    assert 'modconv2d_winograd' not in rec.names and len(fusions) == 1
    placement.forget()
