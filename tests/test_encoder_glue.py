"""The pSp encoder's inference glue on its HIP kernels (csrc/encoder_glue.hip: bn_prelu, se_pool, se_gate, ir_tail) and
the fused body built from them (psp_encoder_model/encoders/helpers.py: fused_units / fused_body).

Per kernel: the aten composite in float64 on the CPU is the exact value, the same composite in fp32 on the GPU is the
reference, and the gate is the project's own (tests/test_hip_forward_b8.py):
    |HIP - fp64| <= 4 |reference fp32 - fp64| + 2e-6 max|fp64|.
Every figure is printed before it is asserted (pytest -s), and two calls must give the same bits.

Shapes: B = 3; C = 64 (C/16 = 4) and C = 96 (C/16 = 6: no power of two, no multiple of 64); 7 x 9 pixels, odd both ways, so
a stride-2 shortcut is 4 x 5; 5 x 7 for se_pool, where the chunks are 3 + 2 rows; 701 x 9 at C = 64 is 2103 work items of
the elementwise kernels against a grid of at most 2048 blocks, so the grid-stride loop makes a second trip, and 234
chunks of se_pool with the pixel-lane loop making several trips; C = 512 makes se_gate's channel loops take two trips.
C = 66 is refused."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import launches
import synth
from gpumem import dev
from parity import closer_to_fp64

pytestmark = pytest.mark.gpu


def _cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _gate(tag, got, ref32, ref64):
    a, r32, r64 = (t.detach().cpu().numpy() for t in (got, ref32, ref64))
    assert a.shape == r64.shape, (tag, a.shape, r64.shape)
    closer_to_fp64(f'GLUE {tag}', a, r32, r64, ref_name='aten32')


def _bn_vectors(name, c):
    """(mean, var, gamma, beta, eps) as fp32 CPU tensors, distributed like tests/synth.py's BatchNorm statistics."""
    return (synth.tensor(name + '/mean', (c,), scale=0.1), synth.tensor(name + '/var', (c,), dist='uniform', scale=0.5, shift=1.0),
            synth.tensor(name + '/gamma', (c,), scale=0.1, shift=1.0), synth.tensor(name + '/beta', (c,), scale=0.1), 1e-5)


def _bn_to(bn, **kw):
    return tuple(v.to(**kw) for v in bn[:4]) + (bn[4],)


def _bn_ref(x, bn):
    return F.batch_norm(x, bn[0], bn[1], bn[2], bn[3], False, 0.0, bn[4])


def _both(fn):
    """fn(convert) evaluated as float64 on the CPU and as fp32 on the GPU; convert moves one input tensor."""
    r64 = fn(lambda t: t.double())
    r32 = fn(lambda t: t.to(dev()))
    return r32, r64


SHAPES = [(3, 64, 7, 9), (3, 96, 7, 9), (3, 64, 701, 9)]
IDS = ['c64', 'c96', 'c64-second-trip']


# ----------------------------------------------------------------------------- bn_prelu
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
@pytest.mark.parametrize('outs', ['y', 'y+next', 'next+sub2', 'y+next+sub2'])
def test_bn_prelu(shape, outs):
    """'next+sub2' is what the encoder's input layer asks for, 'y+next' what it asks for when the first unit has a
    convolution shortcut; 'y' and all three complete the set."""
    from op import _native
    b, c, h, w = shape
    x = synth.tensor('glue/bnp/x', shape)
    bn, nbn = _bn_vectors('glue/bnp/bn', c), _bn_vectors('glue/bnp/next', c)
    slope = synth.tensor('glue/bnp/slope', (c,), scale=0.05, shift=0.25)
    want_y, want_next, s = 'y' in outs.split('+'), 'next' in outs, 2 if 'sub2' in outs else 0

    def run():
        return _native.bn_prelu(_cl(x), _bn_to(bn, device=dev()), slope.to(dev()), want_y=want_y,
                                bn_next=_bn_to(nbn, device=dev()) if want_next else None, sub_stride=s)

    def ref(cv):
        y = F.prelu(_bn_ref(cv(x), tuple(cv(v) for v in bn[:4]) + (bn[4],)), cv(slope))
        return y, _bn_ref(y, tuple(cv(v) for v in nbn[:4]) + (nbn[4],)), y[:, :, ::2, ::2]

    got, again = run(), run()
    r32, r64 = _both(ref)
    for k, name in enumerate(('y', 'y_next', 'y_sub')):
        wanted = (want_y, want_next, s > 0)[k]
        assert (got[k] is not None) == wanted, name
        if wanted:
            assert got[k].shape == r64[k].shape and got[k].permute(0, 2, 3, 1).is_contiguous(), name
            _gate(f'bn_prelu {outs} {shape} {name}', got[k], r32[k], r64[k])
            assert torch.equal(got[k], again[k]), f'{name}: two calls differ'


# ----------------------------------------------------------------------------- se_pool / se_gate
@pytest.mark.parametrize('shape', [(3, 64, 5, 7), (3, 96, 5, 7), (3, 64, 7, 9), (3, 64, 701, 9), (2, 512, 5, 7)],
                         ids=['c64-5x7', 'c96-5x7', 'c64-7x9', 'c64-many-chunks', 'c512'])
def test_se_pool_and_gate(shape):
    from op import _native
    b, c, h, w = shape
    r = synth.tensor('glue/se/r', shape, shift=0.25)
    bn = _bn_vectors('glue/se/bn', c)
    fc1 = synth.tensor('glue/se/fc1', (c // 16, c, 1, 1), scale=(1.0 / c) ** 0.5)
    fc2 = synth.tensor('glue/se/fc2', (c, c // 16, 1, 1), scale=(16.0 / c) ** 0.5)
    chunks = _native.lib().fmgan_se_pool_chunks(b, c, h, w)
    if (h, w) == (5, 7):
        assert chunks == 2, chunks          # 3 + 2 rows: the last chunk is partial
    if h == 701:
        assert chunks > 200, chunks

    def run():
        partial = _native.se_pool(_cl(r))
        return partial, _native.se_gate(partial, h * w, _bn_to(bn, device=dev()), fc1.to(dev()), fc2.to(dev()))

    def ref(cv):
        x = cv(r)
        v = F.adaptive_avg_pool2d(_bn_ref(x, tuple(cv(t) for t in bn[:4]) + (bn[4],)), 1)
        return x.sum((2, 3)), torch.sigmoid(F.conv2d(F.relu(F.conv2d(v, cv(fc1))), cv(fc2))).flatten(1)

    (partial, gate), (partial2, gate2) = run(), run()
    assert tuple(partial.shape) == (b, chunks, c) and tuple(gate.shape) == (b, c)
    r32, r64 = _both(ref)
    _gate(f'se_pool {shape}', partial.sum(1), r32[0], r64[0])
    _gate(f'se_gate {shape}', gate, r32[1], r64[1])
    assert torch.equal(partial, partial2) and torch.equal(gate, gate2), 'two calls differ'


# ----------------------------------------------------------------------------- ir_tail
@pytest.mark.parametrize('with_next', [False, True], ids=['', 'next'])
@pytest.mark.parametrize('with_gate', [False, True], ids=['nogate', 'gate'])
@pytest.mark.parametrize('shortcut', ['identity', 'stride2', 'conv'])
@pytest.mark.parametrize('c', [64, 96])
def test_ir_tail(c, shortcut, with_gate, with_next):
    _ir_tail_case((3, c, 7, 9), shortcut, with_gate, with_next)


@pytest.mark.parametrize('shortcut', ['identity', 'stride2', 'conv'])
def test_ir_tail_second_trip(shortcut):
    _ir_tail_case((3, 64, 1401 if shortcut == 'stride2' else 701, 9), shortcut, True, True)


def _ir_tail_case(in_shape, shortcut, with_gate, with_next):
    """in_shape: the unit's input; the residual branch r has the output's shape (4 x 5 from 7 x 9 at stride 2)."""
    from op import _native
    b, c, hi, wi = in_shape
    s = 2 if shortcut == 'stride2' else 1
    h, w = (hi - 1) // s + 1, (wi - 1) // s + 1
    r = synth.tensor('glue/tail/r', (b, c, h, w))
    src = synth.tensor('glue/tail/src', in_shape)                # the unit's input, or the shortcut convolution's output
    gate = synth.tensor('glue/tail/gate', (b, c), dist='uniform', scale=0.5, shift=0.5)
    bn, sbn, nbn = (_bn_vectors('glue/tail/' + n, c) for n in ('bn', 'sc', 'next'))

    def run():
        return _native.ir_tail(_cl(r), _bn_to(bn, device=dev()), gate.to(dev()) if with_gate else None, _cl(src), s,
                               _bn_to(sbn, device=dev()) if shortcut == 'conv' else None,
                               _bn_to(nbn, device=dev()) if with_next else None)

    def ref(cv):
        t = _bn_ref(cv(r), tuple(cv(v) for v in bn[:4]) + (bn[4],))
        if with_gate:
            t = t * cv(gate)[:, :, None, None]
        if shortcut == 'conv':
            sc = _bn_ref(cv(src), tuple(cv(v) for v in sbn[:4]) + (sbn[4],))
        else:
            sc = F.max_pool2d(cv(src), 1, s)
        out = t + sc
        return out, _bn_ref(out, tuple(cv(v) for v in nbn[:4]) + (nbn[4],))

    got, again = run(), run()
    r32, r64 = _both(ref)
    tag = f'ir_tail {shortcut} gate={with_gate} {tuple(r.shape)}'
    _gate(tag + ' out', got[0], r32[0], r64[0])
    assert torch.equal(got[0], again[0]), 'out: two calls differ'
    assert (got[1] is not None) == with_next
    if with_next:
        _gate(tag + ' out_next', got[1], r32[1], r64[1])
        assert torch.equal(got[1], again[1]), 'out_next: two calls differ'


# ----------------------------------------------------------------------------- refusals
def test_width_66_is_refused_and_the_modules_run():
    from op import _native
    from psp_encoder_model.encoders import helpers
    c = 66
    x = _cl(synth.tensor('glue/66/x', (2, c, 7, 9)))
    bn = _bn_to(_bn_vectors('glue/66/bn', c), device=dev())
    slope = torch.full((c,), 0.25, device=dev())
    L = _native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    v = [t.data_ptr() for t in bn[:4]]
    y = torch.empty_like(x)
    assert L.fmgan_bn_prelu_f32(x.data_ptr(), *v, 1e-5, slope.data_ptr(), y.data_ptr(), None, None, None, None, 0.0, None,
                                None, 2, c, 7, 9, 0, stream) == -2
    assert L.fmgan_se_pool_chunks(2, c, 7, 9) == 0
    assert L.fmgan_se_pool_f32(x.data_ptr(), y.data_ptr(), 2, c, 7, 9, stream) == -2
    assert L.fmgan_se_gate_f32(y.data_ptr(), 1, 63, *v, 1e-5, x.data_ptr(), x.data_ptr(), y.data_ptr(), 2, c, 4, stream) == -2
    assert L.fmgan_ir_tail_f32(x.data_ptr(), *v, 1e-5, None, x.data_ptr(), 7, 9, 1, None, None, None, None, 0.0,
                               y.data_ptr(), None, None, None, None, 0.0, None, 2, c, 7, 9, stream) == -2
    assert _native.bn_prelu(x, bn, slope) is None and _native.se_pool(x) is None
    assert _native.ir_tail(x, bn, None, x) is None
    # bad arguments are refused before any HIP call
    assert L.fmgan_bn_prelu_f32(None, *v, 1e-5, slope.data_ptr(), y.data_ptr(), None, None, None, None, 0.0, None, None,
                                2, 64, 7, 9, 0, stream) == -1
    assert L.fmgan_ir_tail_f32(x.data_ptr(), *v, 1e-5, None, x.data_ptr(), 7, 9, 2, None, None, None, None, 0.0,
                               y.data_ptr(), None, None, None, None, 0.0, None, 2, 64, 7, 9, stream) == -1
    # a body of that width: the fused path declines and the modules give the result
    torch.manual_seed(0)
    body = torch.nn.Sequential(helpers.bottleneck_IR_SE(c, c, 2), helpers.bottleneck_IR_SE(c, c, 1)).to(dev()).eval()
    body = body.to(memory_format=torch.channels_last)
    with torch.no_grad():
        assert helpers.fused_units(body, x) is None
        assert body(x).shape == (2, c, 4, 5)
        wide = torch.nn.Sequential(helpers.bottleneck_IR_SE(64, 64, 2)).to(dev()).eval()
        assert helpers.fused_units(wide, _cl(synth.tensor('glue/66/x64', (2, 64, 7, 9)))) is not None
        assert helpers.fused_units(wide, synth.tensor('glue/66/x64', (2, 64, 7, 9)).to(dev())) is None     # NCHW
    with torch.enable_grad():
        assert helpers.fused_units(wide, _cl(synth.tensor('glue/66/x64', (2, 64, 7, 9)))) is None


# ----------------------------------------------------------------------------- body and whole encoder
def _encoder(n_styles):
    from psp_encoder_model.encoders import psp_encoders
    enc = psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=n_styles))
    enc.load_state_dict(synth.state_dict('psp', enc.state_dict(), seed=7))
    return enc.eval()


def _module_body(body, x, taps):
    feats = {}
    for i, unit in enumerate(body):
        x = unit(x)
        if i in taps:
            feats[i] = x
    return feats


def test_body_fused_vs_modules_vs_fp64():
    """enc.body (eight IR-SE units, synthetic BatchNorm statistics) on [2,64,32,32]: the three pyramid taps of the fused
    path and of the module path, each against the float64 modules on the CPU.  No bit comparison of two calls here: the
    MIOpen convolutions between the glue kernels differ from run to run themselves (1.4e-6 .. 3e-6 absolute at these
    taps, on either path); the kernels' own reproducibility is tested above."""
    from psp_encoder_model.encoders import helpers
    taps = (3, 5, 7)
    enc = _encoder(1)
    x = synth.tensor('glue/body/x', (2, 64, 32, 32))
    with torch.no_grad():
        f64 = _module_body(copy.deepcopy(enc.body).double(), x.double(), taps)
        body = enc.body.to(dev()).to(memory_format=torch.channels_last)
        xg = _cl(x)
        mod = _module_body(body, xg, taps)
        fused = helpers.fused_units(body, xg, taps)
        assert fused is not None, 'the fused path declined the encoder body'
        last, feats = fused
    assert sorted(feats) == list(taps) and last is feats[7]
    for t in taps:
        _gate(f'body tap {t} modules', mod[t], mod[t], f64[t])
        _gate(f'body tap {t} fused', feats[t], mod[t], f64[t])


def test_whole_encoder_fused_vs_switched_off():
    """B = 1 at 256^2, one head per pyramid level and more: fused (the default) against ENCODER_FUSE = False within
    5e-6 max|out|, the tolerance of the encoder goldens (MIOpen's own run-to-run spread is 3.9e-7)."""
    from psp_encoder_model.encoders import helpers
    enc = _encoder(8).to(dev())
    x = synth.tensor('glue/enc/x', (1, 3, 256, 256), dist='uniform').to(dev())
    assert helpers.ENCODER_FUSE, 'the fused path is the default'
    with torch.no_grad(), launches.observed() as rec:
        try:
            a = enc(x)
            fused_names = [n for n in rec.names if n in ('bn_prelu', 'se_pool', 'se_gate', 'ir_tail')]
            del rec.seen[:]
            helpers.ENCODER_FUSE = False
            b = enc(x)
        finally:
            helpers.ENCODER_FUSE = True
    assert fused_names == ['bn_prelu'] + ['se_pool', 'se_gate', 'ir_tail'] * 8, fused_names
    assert not [n for n in rec.names if n in ('bn_prelu', 'se_pool', 'se_gate', 'ir_tail')]
    d, m = float((a - b).abs().max()), float(b.abs().max())
    print(f'GLUE encoder fused vs modules: max|diff| {d:.3e} = {d / m:.3e} of max|out| {m:.3e}', flush=True)
    assert d <= 5e-6 * m
