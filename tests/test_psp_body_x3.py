"""The pSp encoder body's 3x3 convolutions on the split-operand kernel family (csrc/conv3x3_x3.hip:
conv3x3_mfma_bf16x3<stride, channels_last input, epilogue>; op/_native/conv.py: conv3x3_bf16x3; helpers.py:
body_x3_serves / _unit_convs with BODY_X3; psp_encoders.py: the heads' first convolution reading channels_last).

The exact value is float64 F.conv2d(stride, pad 1) + epilogue on the CPU, the reference is the same composite in fp32 on
the GPU (aten / MIOpen) on the same inputs, and the gate is the project's own (parity.closer_to_fp64):
    |HIP - fp64| <= 4 |aten fp32 - fp64| + 2e-6 max|fp64|.
Every figure is printed before it is asserted (pytest -s).

Shapes.  The tile is 64 output channels x (4 rows x 32 columns) of output positions, K in chunks of 16 input channels.
CASES is (batch, cin, cout, h, w, stride, epilogue, channels_last input); every case runs in both output layouts, and the
twelve (stride, epilogue, input layout) instantiations each appear:
  * Cin 8 is one partial chunk, 24 a full and a partial one (with channels_last input: the parked channel quads of the
    ragged chunk), 64 four full ones;
  * Cout 32 and 96 leave the channel tile ragged (half a tile; one and a half), 30 is no multiple of 4 (scalar
    channels_last stores instead of 16-byte ones; both strides);
  * 1 x 1 and 3 x 3 inputs: every tap touches the padding; 5 x 34 is not square, and at stride 1 crosses the 32-column
    tile with a ragged last row tile; 34 x 34 at stride 1 crosses the column tile and has nine row tiles, the last
    ragged; 66 x 66 at stride 2 gives the 33 x 33 output (two column tiles, nine row tiles, both ragged);
  * B = 1 and 3.
The PReLU slope has zero, negative and positive entries; LeakyReLU has a bias vector."""
import copy
import types

import pytest
import torch
import torch.nn.functional as F

import codeobj
import launches
import synth
from gpumem import dev, guarded, guards_intact
from parity import closer_to_fp64, ref_errors, within_reference

gpu = pytest.mark.gpu

SLOPE = 0.01
EPI = {None: 0, 'lrelu': 1, 'prelu': 2}


def _epilogue(y, epi, aux):
    if epi == 'lrelu':
        return F.leaky_relu(y + aux.view(1, -1, 1, 1), SLOPE)
    if epi == 'prelu':
        return F.prelu(y, aux)
    return y


def _ref(x, w, aux, stride, epi, dtype, device):
    y = F.conv2d(x.to(device=device, dtype=dtype), w.to(device=device, dtype=dtype), None, stride, 1)
    return _epilogue(y, epi, None if aux is None else aux.to(device=device, dtype=dtype))


def _hip(x, w, aux, stride, epi, nhwc_in):
    """The NCHW result; the channels_last one (written so by the kernel) must hold the same bits."""
    from op import _native
    xd, wd = x.to(dev()), w.to(dev())
    if nhwc_in:
        xd = xd.contiguous(memory_format=torch.channels_last)
    ad = None if aux is None else aux.to(dev())
    img = _native.conv_weight_to_bf16x3(wd)
    y = _native.conv3x3_bf16x3(xd, img, w.shape[0], stride, epi, ad, SLOPE)
    assert y is not None, 'the library declined the shape'
    ycl = _native.conv3x3_bf16x3(xd, img, w.shape[0], stride, epi, ad, SLOPE, channels_last=True)
    assert y.is_contiguous() and ycl.is_contiguous(memory_format=torch.channels_last) and ycl.shape == y.shape
    assert torch.equal(ycl.view(torch.int32), y.view(torch.int32)), 'channels_last output differs from the NCHW one'
    return y


def _aux(tag, epi, cout):
    if epi == 'lrelu':
        return synth.tensor(f'bx3/{tag}/b', (cout,), scale=0.1)
    if epi == 'prelu':
        s = synth.tensor(f'bx3/{tag}/s', (cout,), scale=0.25)
        s[0], s[1], s[2] = 0.0, -0.5, 0.3
        return s
    return None


def _inputs(tag, b, cin, cout, h, w, epi):
    x = synth.tensor(f'bx3/{tag}/x', (b, cin, h, w))
    wgt = synth.tensor(f'bx3/{tag}/w', (cout, cin, 3, 3), scale=(2.0 / (9 * cin)) ** 0.5)
    return x, wgt, _aux(tag, epi, cout)


CASES = [(1, 8, 32, 1, 1, 1, 'prelu', True), (1, 8, 32, 1, 1, 2, None, False), (3, 24, 96, 3, 3, 1, 'lrelu', False),
         (3, 24, 96, 3, 3, 2, 'prelu', True), (3, 8, 32, 5, 34, 1, None, True), (1, 8, 30, 5, 34, 2, 'lrelu', True),
         (3, 24, 32, 5, 34, 2, 'lrelu', False), (1, 24, 96, 34, 34, 1, 'prelu', True), (1, 64, 32, 34, 34, 1, None, False),
         (1, 24, 32, 34, 34, 1, 'lrelu', True), (1, 8, 32, 66, 66, 2, None, True), (1, 64, 96, 66, 66, 2, 'prelu', False),
         (1, 8, 30, 3, 3, 1, 'prelu', False)]


def _id(c):
    return 'b%d-i%d-o%d-%dx%d-s%d-%s-%s' % (c[:6] + (c[6] or 'none', 'nhwc' if c[7] else 'nchw'))


def test_cases_reach_every_instantiation():
    assert {(c[5], c[6], c[7]) for c in CASES} == {(s, e, n) for s in (1, 2) for e in EPI for n in (False, True)}


@gpu
@pytest.mark.parametrize('case', CASES, ids=[_id(c) for c in CASES])
def test_kernel_vs_fp64(case):
    from op import _native
    b, cin, cout, h, w, stride, epi, nhwc_in = case
    assert _native.conv3x3_bf16x3_supported(b, cin, cout, h, w, stride, nhwc_in)
    x, wgt, aux = _inputs('k', b, cin, cout, h, w, epi)
    r64 = _ref(x, wgt, aux, stride, epi, torch.float64, 'cpu')
    r32 = _ref(x, wgt, aux, stride, epi, torch.float32, dev())
    y = _hip(x, wgt, aux, stride, epi, nhwc_in)
    assert tuple(y.shape) == tuple(r64.shape) == (b, cout, (h - 1) // stride + 1, (w - 1) // stride + 1)
    closer_to_fp64('BX3 conv %s' % _id(case), y.cpu().numpy(), r32.cpu().numpy(), r64.numpy(), ref_name='aten32')
    assert torch.equal(y, _hip(x, wgt, aux, stride, epi, nhwc_in)), 'two calls differ'


@gpu
@pytest.mark.parametrize('shape', [(3, 24, 96, 5, 34), (1, 8, 30, 66, 66)], ids=['i24-o96-5x34', 'i8-o30-66x66'])
def test_channels_last_input_has_the_bits_of_the_heads_kernel(shape):
    """Stride 2 with bias + LeakyReLU: the channels_last-input instantiation against the existing NCHW-input entry point on
    the same values.  The summation order is the same, so any difference is a staging bug."""
    from op import _native
    b, cin, cout, h, w = shape
    x, wgt, bias = _inputs('bits', b, cin, cout, h, w, 'lrelu')
    xd, bd = x.to(dev()), bias.to(dev())
    img = _native.conv_weight_to_bf16x3(wgt.to(dev()))
    old = _native.conv3x3s2_bf16x3(xd, img, bd, cout, SLOPE)
    new = _native.conv3x3_bf16x3(xd.contiguous(memory_format=torch.channels_last), img, cout, 2, 'lrelu', bd, SLOPE)
    via_old_name = _native.conv3x3s2_bf16x3(xd.contiguous(memory_format=torch.channels_last), img, bd, cout, SLOPE)
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))
    assert torch.equal(old.view(torch.int32), via_old_name.view(torch.int32))


# ----------------------------------------------------------------------------- special values
FINITE = [0.0, -0.0, 3.3e38, -3.3e38, 3.4e38, -3.4e38, 1e-38, -1e-38, 1e-39, 1e-40]
NONFINITE = [float('inf'), -float('inf'), float('nan')]
# input positions of the values, by index: the four beyond 1e38 (and Inf, -Inf, NaN, which take the first three of their
# places in channels of their own) sit in the corners, five apart, so no 3 x 3 window — at either stride — holds two of
# them, and the outputs away from the corners stay ordinary
FAR = [(0, 0), (0, 5), (5, 0), (5, 5)]
PLACE = [(1, 1), (1, 4), FAR[0], FAR[1], FAR[2], FAR[3], (4, 1), (4, 4), (2, 2), (3, 3), FAR[0], FAR[1], FAR[2]]


def _special_case(where, values, stride):
    """16 -> 32 channels at 6 x 6; every ordinary operand is uniform in [-0.5, 0.5].  Inputs: value k goes to channel k at
    PLACE[k].  Weights: value k goes to output channel k, input channel k, centre tap (the tap that never meets the
    padding), so it has an output channel of its own.  The slope keeps zero, negative and positive entries."""
    x = synth.tensor(f'bx3/sp/{where}{stride}/x', (1, 16, 6, 6), dist='uniform', scale=0.5)
    wgt = synth.tensor(f'bx3/sp/{where}{stride}/w', (32, 16, 3, 3), dist='uniform', scale=0.5)
    assert float(x.abs().max()) <= 0.5 and float(wgt.abs().max()) <= 0.5
    for k, v in enumerate(values):
        if where == 'input':
            x[0, k, PLACE[k][0], PLACE[k][1]] = v
        else:
            wgt[k, k % 16, 1, 1] = v
    return x, wgt, _aux('sp', 'prelu', 32)


@gpu
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('where', ['input', 'weight'])
@pytest.mark.parametrize('kinds', ['finite', 'all'])
def test_special_values(where, kinds, stride):
    """'finite': +-0, +-3.3e38, +-3.4e38 (beyond the largest bf16: its RNE rounding is Inf) and the 1e-38 .. 1e-40
    neighbourhood stay on the matrix pipe: no Inf or NaN may appear.  'all' adds +-Inf and NaN, which must come out where
    and as F.conv2d + prelu has them (the float64 one: no finite sum overflows here, so its non-finite outputs are those
    of an fp32 direct convolution)."""
    x, wgt, slope = _special_case(where, FINITE + (NONFINITE if kinds == 'all' else []), stride)
    r32 = _ref(x, wgt, slope, stride, 'prelu', torch.float32, dev()).cpu()
    r64 = _ref(x, wgt, slope, stride, 'prelu', torch.float64, 'cpu')
    y = _hip(x, wgt, slope, stride, 'prelu', True).cpu()
    assert torch.equal(_hip(x, wgt, slope, stride, 'prelu', False).cpu().view(torch.int32), y.view(torch.int32))
    fin = torch.isfinite(r64)
    print(f'BX3 special {where}/{kinds}/s{stride}: {int((~fin).sum())} non-finite of {r64.numel()} in fp64, '
          f'{int((~torch.isfinite(r32)).sum())} in aten32, {int((~torch.isfinite(y)).sum())} in HIP; '
          f'NaN {int(torch.isnan(r64).sum())} / {int(torch.isnan(y).sum())}', flush=True)
    if kinds == 'finite':
        assert bool(fin.all()) and float(r64.abs().max()) < 3.4e38, 'the reference itself overflowed: the case is wrong'
    else:
        assert int((~fin).sum()) > 0
    assert torch.equal(torch.isnan(y), torch.isnan(r64))
    inf64, infy = torch.isinf(r64), torch.isinf(y)
    assert torch.equal(infy, inf64) and torch.equal(y[infy].double(), r64[inf64])        # the same Inf, sign included
    fin = fin & torch.isfinite(r32)
    a, b32, b64 = (t[fin].numpy() for t in (y, r32, r64))
    e_hip, e_ref = ref_errors(a, b32, b64)
    print(f'BX3 special {where}/{kinds}/s{stride}: |HIP-fp64| {e_hip:.3e}  |aten32-fp64| {e_ref:.3e} over the finite positions',
          flush=True)
    assert within_reference(e_hip, e_ref), (e_hip, e_ref)
    # the gate above is relative to max|fp64| ~ 1.7e38; the ordinary positions (|out| < 100) on their own scale too
    small = fin & (r64.abs() < 100.0)
    assert int(small.sum()) > 0
    e_hip, e_ref = ref_errors(y[small].numpy(), r32[small].numpy(), r64[small].numpy())
    print(f'BX3 special {where}/{kinds}/s{stride}: |HIP-fp64| {e_hip:.3e}  |aten32-fp64| {e_ref:.3e} over the ordinary positions',
          flush=True)
    assert within_reference(e_hip, e_ref), (e_hip, e_ref)


# ----------------------------------------------------------------------------- refusals, bad arguments, bounds
def _raw(L, x, wts, aux, out, shape, stride, in_nhwc, out_nhwc, epi):
    p = [None if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in (x, wts, aux, out)]
    return L.fmgan_conv3x3_bf16x3_f32(*p, *shape, stride, in_nhwc, out_nhwc, epi, SLOPE, torch.cuda.current_stream().cuda_stream)


@gpu
def test_refused_shapes_return_the_code_and_launch_nothing():
    """One sample's input of 512 x 2048 x 2048 floats is past the 32-bit buffer range, in either layout and at either
    stride; channels_last input with cin % 4 != 0 is declined: the query says 0, the launch returns FMGAN_EUNSUPPORTED and
    the output keeps its fill.  (Raw calls: the tensors are stand-ins, never read.)"""
    from op import _native
    L = _native.lib()
    x = torch.zeros(64, device=dev())
    wts = torch.zeros(64, dtype=torch.int16, device=dev())
    for shape, stride, in_nhwc in (((1, 512, 32, 2048, 2048), 1, 1), ((1, 512, 32, 2048, 2048), 2, 0),
                                   ((1, 512, 32, 2048, 2048), 1, 0), ((1, 6, 8, 4, 4), 1, 1), ((1, 6, 8, 4, 4), 2, 1)):
        assert not _native.conv3x3_bf16x3_supported(*shape, stride, in_nhwc), (shape, stride, in_nhwc)
        buf, out = guarded(64)
        st = _raw(L, x, wts, x, out, shape, stride, in_nhwc, 0, 2)
        torch.cuda.synchronize()
        assert st == _native.FMGAN_EUNSUPPORTED, (shape, stride, in_nhwc, st)
        assert bool(torch.isnan(out).all()) and guards_intact(buf)
    assert _native.conv3x3_bf16x3_supported(1, 6, 8, 4, 4, 1, 0)          # the same width is served from NCHW
    assert not _native.conv3x3_bf16x3_supported(1, 8, 8, 4, 4, 3, 0)      # no such stride


@gpu
def test_bad_arguments_are_einval_and_an_empty_batch_is_ok():
    from op import _native
    L = _native.lib()
    shape = (1, 8, 8, 4, 4)
    x = torch.zeros(8 * 16 + 4, device=dev())
    wts = torch.zeros(54 * 32 * 8, dtype=torch.int16, device=dev())
    buf, out = guarded(8 * 16 + 4)
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    bad = [_raw(L, None, wts, x, out, shape, 1, 0, 0, 0), _raw(L, x, None, x, out, shape, 1, 0, 0, 0),
           _raw(L, x, wts, x, None, shape, 1, 0, 0, 0),
           _raw(L, x, wts, None, out, shape, 1, 0, 0, 2),                         # PReLU without a slope
           _raw(L, x, wts, x, out, shape, 3, 0, 0, 0), _raw(L, x, wts, x, out, shape, 0, 0, 0, 0),   # stride
           _raw(L, x, wts, x, out, shape, 1, 0, 0, 3), _raw(L, x, wts, x, out, shape, 1, 2, 0, 0),   # epilogue, layout flag
           _raw(L, x.data_ptr() + 4, wts, x, out, shape, 1, 1, 0, 0),             # misaligned channels_last input
           _raw(L, x, wts, x, out.data_ptr() + 4, shape, 1, 0, 1, 0),             # misaligned channels_last output
           _raw(L, x, wts, x, out, (1, 0, 8, 4, 4), 1, 0, 0, 0), _raw(L, x, wts, x, out, (-1, 8, 8, 4, 4), 1, 0, 0, 0)]
    torch.cuda.synchronize()
    assert bad == [_native.FMGAN_EINVAL] * len(bad), bad
    assert bool(torch.isnan(out).all()) and guards_intact(buf)
    assert L.fmgan_conv3x3_bf16x3_f32(None, None, None, None, 0, 8, 8, 4, 4, 1, 1, 1, 2, SLOPE, None) == _native.FMGAN_OK


@gpu
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('out_nhwc', [0, 1])
def test_guards_stay_intact_on_ragged_tiles(stride, out_nhwc):
    """[3, 24, 30, 5, 34]: ragged channel tile (30 of 64, scalar channels_last stores), ragged row and column tiles; and
    Cout 96 with the 16-byte stores.  The output lies between guard words and equals the wrapper's."""
    from op import _native
    L = _native.lib()
    for cout in (30, 96):
        b, cin, h, w = 3, 24, 5, 34
        x, wgt, slope = _inputs('guard', b, cin, cout, h, w, 'prelu')
        xd = x.to(dev()).contiguous(memory_format=torch.channels_last)
        sd = slope.to(dev())
        img = _native.conv_weight_to_bf16x3(wgt.to(dev()))
        want = _native.conv3x3_bf16x3(xd, img, cout, stride, 'prelu', sd, channels_last=bool(out_nhwc))
        oh, ow = want.shape[2:]
        buf, out = guarded((b, oh, ow, cout) if out_nhwc else (b, cout, oh, ow))
        assert out.data_ptr() % 16 == 0
        st = _raw(L, xd, img, sd, out, (b, cin, cout, h, w), stride, 1, out_nhwc, 2)
        torch.cuda.synchronize()
        assert st == _native.FMGAN_OK and guards_intact(buf)
        got = out.permute(0, 3, 1, 2) if out_nhwc else out
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ----------------------------------------------------------------------------- unit, body, encoder
_ENC = {}


def _encoder(n_styles):
    from psp_encoder_model.encoders import psp_encoders
    if n_styles not in _ENC:
        enc = psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=n_styles))
        enc.load_state_dict(synth.state_dict('psp', enc.state_dict(), seed=7))
        _ENC[n_styles] = enc.eval()
    return copy.deepcopy(_ENC[n_styles])


def _rule(body, b, hw):
    """The launches the shape rule asks for on a [b, 64, hw, hw] input, as the bracket's infos, and the served conv1s."""
    from psp_encoder_model.encoders import helpers
    infos, served1 = [], []
    for i, unit in enumerate(body):
        c1, c2 = unit.res_layer[1], unit.res_layer[3]
        if hw >= helpers.BODY_X3_MIN_OUT:
            infos.append((b, c1.in_channels, c1.out_channels, hw, hw, 1, EPI['prelu']))
            served1.append(i)
        s = c2.stride[0]
        if (hw - 1) // s + 1 >= helpers.BODY_X3_MIN_OUT:
            infos.append((b, c2.in_channels, c2.out_channels, hw, hw, s, EPI[None]))
        hw = (hw - 1) // s + 1
    return infos, served1


@gpu
def test_body_switch_on_vs_off_vs_fp64():
    """enc.body on [2, 64, 64, 64] channels_last: units 0 and 1 and conv1 of unit 2 (outputs 64 and 32 wide) take the
    kernel, everything after (16 wide and less) stays on MIOpen + aten PReLU.  Switch on against switch off (the fp32
    reference) against the float64 modules at the three pyramid taps; the bracket's infos are the rule's; the PReLU module
    of a served conv1 never runs; switched off the bracket does not appear.  Weight images: kept across forwards, rebuilt
    after weight.copy_."""
    from psp_encoder_model.encoders import helpers
    taps = (3, 5, 7)
    enc = _encoder(1)
    x = synth.tensor('bx3/body/x', (2, 64, 64, 64))
    assert helpers.BODY_X3 and helpers.ENCODER_FUSE, 'the split-operand body is the default'
    with torch.no_grad():
        f64, xx = {}, x.double()
        for i, unit in enumerate(copy.deepcopy(enc.body).double()):
            xx = unit(xx)
            if i in taps:
                f64[i] = xx
        body = enc.body.to(dev()).to(memory_format=torch.channels_last)
        xg = x.to(dev()).contiguous(memory_format=torch.channels_last)
        want, served1 = _rule(body, 2, 64)
        assert want == [(2, 64, 64, 64, 64, 1, 2), (2, 64, 64, 64, 64, 2, 0), (2, 64, 64, 32, 32, 1, 2),
                        (2, 64, 64, 32, 32, 1, 0), (2, 64, 128, 32, 32, 1, 2)] and served1 == [0, 1, 2]
        prelu_runs = []
        hooks = [u.res_layer[2].register_forward_hook(lambda m, a, o, i=i: prelu_runs.append(i)) for i, u in enumerate(body)]
        with launches.observed() as rec:
            last, on = helpers.fused_units(body, xg, taps)
            assert rec.infos('conv3x3_bf16x3') == want, rec.infos('conv3x3_bf16x3')
            assert rec.count('conv_weight_bf16x3') == len(want)
            assert prelu_runs == [i for i in range(len(body)) if i not in served1], prelu_runs
            last2, on2 = helpers.fused_units(body, xg, taps)                    # the kept weight images
            assert rec.count('conv3x3_bf16x3') == 2 * len(want) and rec.count('conv_weight_bf16x3') == len(want)
            w1 = body[1].res_layer[1].weight
            w1.copy_(w1.clone())                                                # what load_state_dict does: one rebuild
            last3, on3 = helpers.fused_units(body, xg, taps)
            assert rec.count('conv_weight_bf16x3') == len(want) + 1
            del rec.seen[:], prelu_runs[:]
            try:
                helpers.BODY_X3 = False
                lastoff, off = helpers.fused_units(body, xg, taps)
            finally:
                helpers.BODY_X3 = True
            assert rec.count('conv3x3_bf16x3') == 0 and rec.count('conv_weight_bf16x3') == 0
            assert prelu_runs == list(range(len(body)))
        for h in hooks:
            h.remove()
    for t in taps:
        assert on[t].shape == off[t].shape and on[t].permute(0, 2, 3, 1).is_contiguous()
        closer_to_fp64(f'BX3 body tap {t} on', on[t].cpu().numpy(), off[t].cpu().numpy(), f64[t].numpy(), ref_name='MIOpen32')
        closer_to_fp64(f'BX3 body tap {t} on (rebuilt image)', on3[t].cpu().numpy(), off[t].cpu().numpy(), f64[t].numpy(),
                       ref_name='MIOpen32')


@gpu
def test_whole_encoder_switch_on_vs_off():
    """E_W_Plus at B = 1, 256^2, 8 heads: thirteen of the body's sixteen convolutions take the kernel (the three at 16^2
    stay), the one fine head reads its channels_last feature map without an NCHW copy; switched off nobody takes the
    body's bracket, and the latents agree within 5e-6 max|out|, the tolerance of the encoder goldens."""
    from psp_encoder_model.encoders import helpers
    enc = _encoder(8).to(dev())
    x = synth.tensor('bx3/enc/x', (1, 3, 256, 256), dist='uniform').to(dev())
    fine_args = []
    hook = enc.styles[7].register_forward_pre_hook(lambda m, args: fine_args.append(args))
    with torch.no_grad(), launches.observed() as rec:
        a = enc(x)
        hook.remove()
        infos = rec.infos('conv3x3_bf16x3')
        heads = rec.infos('conv3x3s2_bf16x3')
        del rec.seen[:]
        try:
            helpers.BODY_X3 = False
            b = enc(x)
        finally:
            helpers.BODY_X3 = True
        assert rec.count('conv3x3_bf16x3') == 0 and rec.infos('conv3x3s2_bf16x3') == heads
    assert infos == _rule(enc.body, 1, 256)[0] and len(infos) == 13, infos
    assert heads == [(1, 512, 512, 64, 64)], heads
    # the fine head got the level's channels_last map itself and no NCHW copy of it
    (feat, nchw), = fine_args
    assert nchw is None and feat.permute(0, 2, 3, 1).is_contiguous() and not feat.is_contiguous()
    d, m = float((a - b).abs().max()), float(b.abs().max())
    print(f'BX3 encoder on vs off: max|diff| {d:.3e} = {d / m:.3e} of max|out| {m:.3e}', flush=True)
    assert d <= 5e-6 * m


@gpu
def test_head_first_conv_reads_channels_last_with_the_bits_of_the_nchw_copy():
    """GradualStyleBlock._first_x3 on a channels_last feature map (read as it is) against the same map copied to NCHW,
    and forward(x) against forward(x, x_nchw) up to the first convolution: the same launch info, the same bits."""
    from psp_encoder_model.encoders import psp_encoders
    blk = psp_encoders.GradualStyleBlock(64, 64, 64)
    blk.convs[0].weight.data = synth.tensor('bx3/head/w', (64, 64, 3, 3), scale=(2.0 / 576) ** 0.5)
    blk.convs[0].bias.data = synth.tensor('bx3/head/b', (64,), scale=0.1)
    blk = blk.to(dev())
    xg = synth.tensor('bx3/head/x', (2, 64, 64, 64)).to(dev()).contiguous(memory_format=torch.channels_last)
    assert psp_encoders.X3_HEAD_CHANNELS_LAST_IN and blk.x3_reads(xg) and not blk.x3_reads(xg.contiguous())
    with torch.no_grad(), launches.observed() as rec:
        assert blk.x3_serves(xg)
        a = blk._first_x3(xg)
        b = blk._first_x3(xg.contiguous())
        assert rec.infos('conv3x3s2_bf16x3') == [(2, 64, 64, 64, 64)] * 2
    assert a.shape == b.shape == (2, 64, 32, 32) and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ----------------------------------------------------------------------------- code object (no GPU)
def test_new_instantiations_do_not_spill(tmp_path):
    """The twelve members of the family, from the code object's notes: no spilled register, no scratch, and the register
    count of the blocks per CU each is built for (stride 1: three, 170; stride 2: two, 256)."""
    kernels = codeobj.kernel_notes(tmp_path)
    names = [k for k in kernels if 'conv3x3_mfma_bf16x3' in k]
    assert len(names) == 12, names
    for n in names:
        k = kernels[n]
        assert k['vgpr_spill'] == 0 and k['scratch'] == 0, (n, k)
        assert k['vgpr'] <= (170 if 'bf16x3ILi1E' in n else 256), (n, k)
    assert not [k for k in kernels if 'conv3x3' in k and 'modconv_mfma_bf16' in k]
