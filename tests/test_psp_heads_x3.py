"""The pSp style heads' first convolution on the split-operand kernel (csrc/conv3x3_x3.hip: conv3x3_mfma_bf16x3<2, NCHW in, LeakyReLU>;
op/_native/conv.py: conv3x3s2_bf16x3, conv_weight_to_bf16x3; op/live_weights.py: split_conv_weight; psp_encoders.py:
GradualStyleBlock with HEADS_X3).

The exact value is float64 F.conv2d(stride 2, pad 1) + bias + LeakyReLU(0.01) on the CPU, the reference is the same
composite in fp32 on the GPU (aten / MIOpen) on the same inputs, and the gate is the project's own
(tests/test_encoder_glue.py):
    |HIP - fp64| <= 4 |aten fp32 - fp64| + 2e-6 max|fp64|.
Every figure is printed before it is asserted (pytest -s).

Shapes.  The kernel's tile is 64 output channels x (4 rows x 32 columns) of output positions, K in chunks of 16 input
channels: Cin 8 is one partial chunk, 24 a full and a partial one, 512 the heads' depth (at 8^2 -> 4^2); Cout 32 and 96
leave the channel tile ragged (half a tile; one and a half), 512 is eight tiles; H = W = 2 gives a 1 x 1 output, 5 and 6
an odd and an even size with the same 3 x 3 output, 16 two row tiles, 34 a 17 x 17 output (five row tiles, the last
ragged) and 66 a 33 x 33 one, which also crosses the 32-column tile; 5 x 34 is not square; Cout 30 is no multiple of 4
(the channels_last output then takes scalar stores, not 16-byte ones).  Every case is computed in both output layouts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import launches
import synth
from gpumem import dev, guarded, guards_intact
from parity import closer_to_fp64, ref_errors, within_reference

pytestmark = pytest.mark.gpu

SLOPE = 0.01


def _ref(x, w, b, dtype, device):
    y = F.conv2d(x.to(device=device, dtype=dtype), w.to(device=device, dtype=dtype), b.to(device=device, dtype=dtype), 2, 1)
    return F.leaky_relu(y, SLOPE)


def _hip(x, w, b):
    """The NCHW result; the channels_last one (written so by the kernel) must hold the same bits."""
    from op import _native
    xd, wd, bd = x.to(dev()), w.to(dev()), b.to(dev())
    img = _native.conv_weight_to_bf16x3(wd)
    y = _native.conv3x3s2_bf16x3(xd, img, bd, w.shape[0], SLOPE)
    assert y is not None, 'the library declined the shape'
    ycl = _native.conv3x3s2_bf16x3(xd, img, bd, w.shape[0], SLOPE, channels_last=True)
    assert y.is_contiguous() and ycl.is_contiguous(memory_format=torch.channels_last) and ycl.shape == y.shape
    assert torch.equal(ycl.view(torch.int32), y.view(torch.int32)), 'channels_last output differs from the NCHW one'
    return y


def _inputs(tag, b, cin, cout, h, w):
    x = synth.tensor(f'x3/{tag}/x', (b, cin, h, w))
    wgt = synth.tensor(f'x3/{tag}/w', (cout, cin, 3, 3), scale=(2.0 / (9 * cin)) ** 0.5)
    bias = synth.tensor(f'x3/{tag}/b', (cout,), scale=0.1)
    return x, wgt, bias


CASES = [(1, 8, 32, 2, 2), (3, 24, 96, 5, 5), (1, 24, 32, 6, 6), (3, 8, 96, 16, 16), (1, 24, 96, 34, 34), (3, 8, 32, 5, 34),
         (1, 8, 32, 66, 66), (1, 512, 512, 8, 8), (3, 512, 32, 8, 8), (1, 8, 30, 6, 6)]


@pytest.mark.parametrize('case', CASES, ids=['b%d-i%d-o%d-%dx%d' % c for c in CASES])
def test_kernel_vs_fp64(case):
    from op import _native
    b, cin, cout, h, w = case
    assert _native.conv3x3s2_bf16x3_supported(*case)
    x, wgt, bias = _inputs('k', *case)
    r64 = _ref(x, wgt, bias, torch.float64, 'cpu')
    r32 = _ref(x, wgt, bias, torch.float32, dev())
    y = _hip(x, wgt, bias)
    assert tuple(y.shape) == tuple(r64.shape) == (b, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    closer_to_fp64('X3 conv %s' % (case,), y.cpu().numpy(), r32.cpu().numpy(), r64.numpy(), ref_name='aten32')
    assert torch.equal(y, _hip(x, wgt, bias)), 'two calls differ'


def test_refused_shape_returns_the_code_and_launches_nothing():
    """One sample's input of 512 x 2048 x 2048 floats is past the 32-bit buffer range: the query says 0, the launch
    returns FMGAN_EUNSUPPORTED and the output keeps its fill.  (Raw call: the tensors are stand-ins, never read.)"""
    from op import _native
    L = _native.lib()
    shape = (1, 512, 32, 2048, 2048)
    assert not _native.conv3x3s2_bf16x3_supported(*shape)
    x = torch.zeros(64, device=dev())
    wts = torch.zeros(64, dtype=torch.int16, device=dev())
    buf, out = guarded(64)
    st = L.fmgan_conv3x3s2_bf16x3_f32(x.data_ptr(), wts.data_ptr(), None, out.data_ptr(), *shape, SLOPE, 0,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == _native.FMGAN_EUNSUPPORTED
    assert bool(torch.isnan(out).all()) and guards_intact(buf)
    assert L.fmgan_conv3x3s2_bf16x3_f32(None, None, None, None, 0, 8, 8, 4, 4, SLOPE, 0, None) == _native.FMGAN_OK   # empty batch
    assert L.fmgan_conv3x3s2_bf16x3_f32(None, None, None, None, 1, 0, 8, 4, 4, SLOPE, 0, None) not in (
        _native.FMGAN_OK, _native.FMGAN_EUNSUPPORTED)


# ----------------------------------------------------------------------------- special values
FINITE = [0.0, -0.0, 3.3e38, -3.3e38, 3.4e38, -3.4e38, 1e-38, -1e-38, 1e-39, 1e-40]
NONFINITE = [float('inf'), -float('inf'), float('nan')]


def _special_case(where, values):
    """16 -> 32 channels at 6 x 6 (3 x 3 outputs); every ordinary operand is uniform in [-0.5, 0.5].  Inputs: value k goes
    to channel k at an EVEN (y, x), which feeds exactly one output position (y/2, x/2) — no two large values meet in one
    sum (+-3.3e38 and +-3.4e38 have positions of their own; Inf, -Inf and NaN share theirs with -0, 3.3e38 and -3.3e38,
    which they swamp).  Weights: value k goes to
    output channel k, input channel k, centre tap (the tap that never meets the padding), so it has an output channel of
    its own."""
    x = synth.tensor(f'x3/sp/{where}/x', (1, 16, 6, 6), dist='uniform', scale=0.5)
    wgt = synth.tensor(f'x3/sp/{where}/w', (32, 16, 3, 3), dist='uniform', scale=0.5)
    bias = synth.tensor(f'x3/sp/{where}/b', (32,), scale=0.1)
    assert float(x.abs().max()) <= 0.5 and float(wgt.abs().max()) <= 0.5
    for k, v in enumerate(values):
        if where == 'input':
            x[0, k, 2 * ((k % 9) // 3), 2 * (k % 3)] = v
        else:
            wgt[k, k % 16, 1, 1] = v
    return x, wgt, bias


@pytest.mark.parametrize('where', ['input', 'weight'])
@pytest.mark.parametrize('kinds', ['finite', 'all'])
def test_special_values(where, kinds):
    """'finite': +-0, +-3.3e38, +-3.4e38 (beyond the largest bf16: its RNE rounding is Inf) and the 1e-38 .. 1e-40
    neighbourhood stay on the matrix pipe: no Inf or NaN may appear.  'all' adds +-Inf and NaN, which must come out where
    and as the fp32 convolution has them."""
    x, wgt, bias = _special_case(where, FINITE + (NONFINITE if kinds == 'all' else []))
    r32 = _ref(x, wgt, bias, torch.float32, dev()).cpu()
    r64 = _ref(x, wgt, bias, torch.float64, 'cpu')
    y = _hip(x, wgt, bias).cpu()
    fin = torch.isfinite(r32)
    print(f'X3 special {where}/{kinds}: {int((~fin).sum())} non-finite of {r32.numel()} in aten32, '
          f'{int((~torch.isfinite(y)).sum())} in HIP; NaN {int(torch.isnan(r32).sum())} / {int(torch.isnan(y).sum())}', flush=True)
    if kinds == 'finite':
        assert bool(fin.all()), 'the fp32 reference itself overflowed: the case is wrong'
    else:
        assert int((~fin).sum()) > 0
    assert torch.equal(torch.isnan(y), torch.isnan(r32))
    inf32, infy = torch.isinf(r32), torch.isinf(y)
    assert torch.equal(infy, inf32) and torch.equal(y[infy], r32[inf32])        # the same Inf, sign included
    a, b32, b64 = (t[fin].numpy() for t in (y, r32, r64))
    e_hip, e_ref = ref_errors(a, b32, b64)
    print(f'X3 special {where}/{kinds}: |HIP-fp64| {e_hip:.3e}  |aten32-fp64| {e_ref:.3e} over the finite positions', flush=True)
    assert within_reference(e_hip, e_ref), (e_hip, e_ref)
    if kinds == 'finite':
        # the gate above is relative to max|fp64| ~ 1.7e38; the ordinary positions (|out| < 100) on their own scale too
        small = r64.abs() < 100.0
        e_hip, e_ref = ref_errors(y[small].numpy(), r32[small].numpy(), r64[small].numpy())
        print(f'X3 special {where}/{kinds}: |HIP-fp64| {e_hip:.3e}  |aten32-fp64| {e_ref:.3e} over the ordinary positions', flush=True)
        assert within_reference(e_hip, e_ref), (e_hip, e_ref)
    assert torch.equal(_hip(x, wgt, bias).cpu().view(torch.int32), y.view(torch.int32)), 'two calls differ'


def test_split_weight_pieces_are_finite_and_exact():
    """modconv_weight_to_bf16x3 on the special weights: no piece of a finite weight is Inf or NaN, the three pieces add up
    to the weight again (up to 2^-126, the smallest normal, where a piece of a weight near it is flushed), +-0 gives zeros,
    and Inf / NaN stay in the high piece alone."""
    from op import _native
    vals = FINITE + NONFINITE
    wt = torch.zeros(16, 1, 32)
    wt[:len(vals), 0, 0] = torch.tensor(vals)
    img = _native.modconv_weight_to_bf16x3(wt.to(dev())).cpu()
    # image [chunk = 1][piece 3][tap 1][k-half 2][row 32][8]: weight (k, row 0) sits at [piece][k // 8][0][k % 8]
    pieces = (img.view(3, 2, 32, 8)[:, :, 0, :].reshape(3, 16).to(torch.int32) << 16).view(torch.float32)
    for k, v in enumerate(vals):
        hi, mid, lo = (float(pieces[j, k]) for j in range(3))
        if np.isfinite(v):
            assert all(np.isfinite(t) for t in (hi, mid, lo)), (v, hi, mid, lo)
            total = float(np.float32(np.float32(hi) + np.float32(mid)) + np.float32(lo))
            if abs(v) >= 1e-30:
                assert total == float(np.float32(v)), (v, hi, mid, lo)
            else:       # pieces below the smallest normal may be flushed: at most 2^-126 is lost
                assert abs(total - float(np.float32(v))) <= 2.0 ** -126, (v, hi, mid, lo)
            if v == 0.0:
                assert hi == 0.0 and mid == 0.0 and lo == 0.0
        else:
            assert (np.isnan(hi) if np.isnan(v) else hi == v) and mid == 0.0 and lo == 0.0, (v, hi, mid, lo)


# ----------------------------------------------------------------------------- the weight image, kept per parameter
def test_weight_image_is_rebuilt_when_the_parameter_changes_and_not_otherwise():
    from op import _native
    from op.live_weights import split_conv_weight
    conv = torch.nn.Conv2d(16, 32, 3, 2, 1).to(dev())
    with torch.no_grad(), launches.observed() as rec:
        a = split_conv_weight(conv)
        assert split_conv_weight(conv) is a and rec.count('conv_weight_bf16x3') == 1
        assert rec.infos('conv_weight_bf16x3') == [(32, 16, 9)]
        conv.weight.mul_(2.0)                                   # in place on the parameter: _version moves
        b = split_conv_weight(conv)
        assert rec.count('conv_weight_bf16x3') == 2 and b is not a
        assert torch.equal(b, _native.conv_weight_to_bf16x3(conv.weight)) and not torch.equal(a, b)
        n = rec.count('conv_weight_bf16x3')
        assert split_conv_weight(conv) is b and rec.count('conv_weight_bf16x3') == n
        conv.weight.data = conv.weight.data.clone() * 0.5       # new storage
        c = split_conv_weight(conv)
        assert rec.count('conv_weight_bf16x3') == n + 1
        assert torch.equal(c, a)                                # (x * 2) * 0.5: the first weights again
        assert split_conv_weight(conv) is c and rec.count('conv_weight_bf16x3') == n + 1
        conv.weight.copy_(torch.zeros_like(conv.weight))        # what load_state_dict does
        split_conv_weight(conv)
        assert rec.count('conv_weight_bf16x3') == n + 2


# ----------------------------------------------------------------------------- module level
def test_style_block_switch_on_vs_off_vs_fp64():
    """GradualStyleBlock(512, 512, 64) at B = 2 on a channels_last feature map: the default (first conv on the
    split-operand kernel, once) against FMGAN_PSP_HEADS_X3 off (MIOpen) as the fp32 reference, both against the float64
    module on the CPU."""
    import copy
    from psp_encoder_model.encoders import psp_encoders
    blk = psp_encoders.GradualStyleBlock(512, 512, 64)
    sd = {}
    for k, v in blk.state_dict().items():
        if k.startswith('convs') and k.endswith('weight'):
            sd[k] = synth.tensor('x3/blk/' + k, tuple(v.shape), scale=(2.0 / 4608) ** 0.5)
        elif k.startswith('convs'):
            sd[k] = synth.tensor('x3/blk/' + k, tuple(v.shape), scale=0.1)
        else:
            sd[k] = synth.tensor('x3/blk/' + k, tuple(v.shape), scale=0.0 if k.endswith('bias') else 1.0)
    blk.load_state_dict(sd)
    x = synth.tensor('x3/blk/x', (2, 512, 64, 64))
    assert psp_encoders.HEADS_X3, 'the split-operand first conv is the default'
    with torch.no_grad():
        r64 = copy.deepcopy(blk).double()(x.double())
        g = blk.to(dev())
        xg = x.to(dev()).contiguous(memory_format=torch.channels_last)
        assert g.x3_serves(xg)
        with launches.observed() as rec:
            on = g(xg)
            assert rec.count('conv3x3s2_bf16x3') == 1 and rec.infos('conv3x3s2_bf16x3') == [(2, 512, 512, 64, 64)]
            assert rec.count('conv_weight_bf16x3') == 1
            on2 = g(xg, xg.contiguous())                         # the level's shared NCHW copy; the kept weight image
            assert rec.count('conv3x3s2_bf16x3') == 2 and rec.count('conv_weight_bf16x3') == 1
            try:
                psp_encoders.HEADS_X3 = False
                assert not g.x3_serves(xg)
                off = g(xg)
            finally:
                psp_encoders.HEADS_X3 = True
            assert rec.count('conv3x3s2_bf16x3') == 2
    d = float((on - on2).abs().max())
    print(f'X3 block: own NCHW copy vs shared one: max|diff| {d:.3e}', flush=True)
    closer_to_fp64('X3 block on', on.cpu().numpy(), off.cpu().numpy(), r64.numpy(), ref_name='MIOpen32')
    closer_to_fp64('X3 block on (shared copy)', on2.cpu().numpy(), off.cpu().numpy(), r64.numpy(), ref_name='MIOpen32')


def test_encoder_takes_the_kernel_once_per_fine_head_and_one_copy_per_level():
    """E_W_Plus at 256^2 (pyramid 16^2 / 32^2 / 64^2), 10 heads: the three fine heads (64^2 -> 32^2) take the kernel, once
    each; the coarse and middle ones (outputs 8 and 16 wide) stay on MIOpen; switched off, nobody takes it and the
    latents agree within 5e-6 max|out|, the tolerance of the encoder goldens."""
    import types
    from psp_encoder_model.encoders import psp_encoders
    enc = psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=10))
    enc.load_state_dict(synth.state_dict('psp', enc.state_dict(), seed=7))
    enc = enc.to(dev()).eval()
    x = synth.tensor('x3/enc/x', (1, 3, 256, 256), dist='uniform').to(dev())
    with torch.no_grad(), launches.observed() as rec:
        a = enc(x)
        infos = rec.infos('conv3x3s2_bf16x3')
        del rec.seen[:]
        try:
            psp_encoders.HEADS_X3 = False
            b = enc(x)
        finally:
            psp_encoders.HEADS_X3 = True
        assert rec.count('conv3x3s2_bf16x3') == 0
    assert infos == [(1, 512, 512, 64, 64)] * 3, infos
    d, m = float((a - b).abs().max()), float(b.abs().max())
    print(f'X3 encoder on vs off: max|diff| {d:.3e} = {d / m:.3e} of max|out| {m:.3e}', flush=True)
    assert d <= 5e-6 * m
