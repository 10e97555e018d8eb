"""The pSp style heads' 16- and 8-wide stride-2 convolutions on the narrow-tile members of the split-operand family
(csrc/conv3x3_x3.hip: conv3x3_tail_x3<16>, <8>; op/_native/conv.py: conv3x3_tail_bf16x3, conv3x3_tail_bf16x3_select;
psp_encoders.py: GradualStyleBlock with TAIL_X3 / TAIL_X3_WIDTHS).

The existing kernel conv3x3_mfma_bf16x3<2, channels_last in, LeakyReLU> serves these shapes already (with half or a
quarter of its position lanes filled), and per output element the narrow tile adds the same products in the same order:
on finite operands the two must agree bit for bit.  Against the exact value (float64 F.conv2d + bias + LeakyReLU on the
CPU) the gate is the project's own, |HIP - fp64| <= 4 |MIOpen fp32 - fp64| + 2e-6 max|fp64|; every figure is printed
before it is asserted (pytest -s).

Shapes (B, cin, cout, h, w), channels_last in and out.  TW = 16 tile: 64 channels x (4 rows x 16 columns), TW = 8: 64 x
(8 x 8), K in chunks of 16 input channels: (2, 32, 64, 32, 32) full 16-wide tiles, four row tiles; (2, 20, 40, 31, 31) a
partial last chunk and a partial channel tile; (1, 16, 30, 29, 32) 15 rows and cout % 4 != 0 (scalar stores);
(2, 16, 64, 20, 18) 10 x 9: the narrowest 16-class width, ragged row tile; (3, 16, 32, 16, 16) a full 8-wide tile;
(2, 36, 64, 15, 13) 8 x 7; (1, 16, 64, 10, 9) 5 x 5, the narrowest width served."""
import copy
import types

import pytest
import torch
import torch.nn.functional as F

import codeobj
import launches
import synth
from gpumem import dev
from parity import closer_to_fp64, ref_errors, within_reference

gpu = pytest.mark.gpu

SLOPE = 0.01
CASES = [(2, 32, 64, 32, 32), (2, 20, 40, 31, 31), (1, 16, 30, 29, 32), (2, 16, 64, 20, 18), (3, 16, 32, 16, 16),
         (2, 36, 64, 15, 13), (1, 16, 64, 10, 9)]
IDS = ['b%d-i%d-o%d-%dx%d' % c for c in CASES]


def _inputs(tag, b, cin, cout, h, w):
    x = synth.tensor(f'tail/{tag}/x', (b, cin, h, w))
    wgt = synth.tensor(f'tail/{tag}/w', (cout, cin, 3, 3), scale=(2.0 / (9 * cin)) ** 0.5)
    bias = synth.tensor(f'tail/{tag}/b', (cout,), scale=0.1)
    return x, wgt, bias


def _ref(x, w, b, dtype, device):
    y = F.conv2d(x.to(device=device, dtype=dtype), w.to(device=device, dtype=dtype), b.to(device=device, dtype=dtype), 2, 1)
    return F.leaky_relu(y, SLOPE)


def _tail(x, w, b, channels_last=True):
    from op import _native
    xd = x.to(dev()).contiguous(memory_format=torch.channels_last)
    img = _native.conv_weight_to_bf16x3(w.to(dev()), 'conv_tail_weight_bf16x3')
    y = _native.conv3x3_tail_bf16x3(xd, img, b.to(dev()), w.shape[0], SLOPE, channels_last=channels_last)
    assert y is not None, 'the library declined the shape'
    assert y.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    return y


# ----------------------------------------------------------------------------- 1. the bits of the existing kernel
@gpu
@pytest.mark.parametrize('channels_last', [True, False], ids=['nhwc-out', 'nchw-out'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_bits_of_the_existing_kernel(case, channels_last):
    from op import _native
    b, cin, cout, h, w = case
    ow = (w - 1) // 2 + 1
    assert _native.conv3x3_tail_bf16x3_select(*case) == (16 if ow > 8 else 8)
    x, wgt, bias = _inputs('bits', *case)
    xd = x.to(dev()).contiguous(memory_format=torch.channels_last)
    img = _native.conv_weight_to_bf16x3(wgt.to(dev()))
    old = _native.conv3x3_bf16x3(xd, img, cout, 2, 'lrelu', bias.to(dev()), SLOPE, channels_last=channels_last)
    new = _tail(x, wgt, bias, channels_last)
    assert old is not None and new.shape == old.shape == (b, cout, (h - 1) // 2 + 1, ow) and new.stride() == old.stride()
    assert bool(torch.isfinite(old).all())
    assert torch.equal(new.view(torch.int32), old.view(torch.int32)), int((new != old).sum())


# ----------------------------------------------------------------------------- 2. against float64; 4. two calls
@gpu
@pytest.mark.parametrize('case', [(2, 512, 512, 32, 32), (2, 512, 512, 16, 16)], ids=['16-wide', '8-wide'])
def test_kernel_vs_fp64_and_two_calls_same_bits(case):
    x, wgt, bias = _inputs('k', *case)
    r64 = _ref(x, wgt, bias, torch.float64, 'cpu')
    r32 = _ref(x.to(dev()).contiguous(memory_format=torch.channels_last), wgt, bias, torch.float32, dev())
    y = _tail(x, wgt, bias)
    closer_to_fp64('TAIL conv %s' % (case,), y.cpu().numpy(), r32.cpu().numpy(), r64.numpy(), ref_name='MIOpen32')
    assert torch.equal(y.view(torch.int32), _tail(x, wgt, bias).view(torch.int32)), 'two calls differ'


# ----------------------------------------------------------------------------- 3. special values
FINITE = [0.0, -0.0, 3.3e38, -3.3e38, 3.4e38, -3.4e38, 1e-38, -1e-38, 1e-39, 1e-40]
NONFINITE = [float('inf'), -float('inf'), float('nan')]


def _special_case(where, values):
    """16 -> 32 channels at 12 x 12 (6 x 6 outputs, the 8-wide class); every ordinary operand is uniform in [-0.5, 0.5].
    Inputs: value k goes to channel k at the even position (2 (k // 4), 2 (k % 4)), which feeds exactly one output
    position, its own: no two special values meet in one sum.  Weights: value k goes to output channel k, input channel
    k, centre tap (the tap that never meets the padding)."""
    x = synth.tensor(f'tail/sp/{where}/x', (1, 16, 12, 12), dist='uniform', scale=0.5)
    wgt = synth.tensor(f'tail/sp/{where}/w', (32, 16, 3, 3), dist='uniform', scale=0.5)
    bias = synth.tensor(f'tail/sp/{where}/b', (32,), scale=0.1)
    assert float(x.abs().max()) <= 0.5 and float(wgt.abs().max()) <= 0.5 and len(values) <= 16
    for k, v in enumerate(values):
        if where == 'input':
            x[0, k, 2 * (k // 4), 2 * (k % 4)] = v
        else:
            wgt[k, k, 1, 1] = v
    return x, wgt, bias


@gpu
@pytest.mark.parametrize('where', ['input', 'weight'])
@pytest.mark.parametrize('kinds', ['finite', 'all'])
def test_special_values(where, kinds):
    """'finite': +-0, +-3.3e38, +-3.4e38 (beyond the largest bf16) and 1e-38 .. 1e-40 stay on the matrix pipe: no Inf or
    NaN appears and the ordinary positions stay within the gate.  'all' adds +-Inf and NaN: the non-finite outputs of
    F.conv2d (fp32) appear at the same positions with the same values."""
    x, wgt, bias = _special_case(where, FINITE + (NONFINITE if kinds == 'all' else []))
    r32 = _ref(x.to(dev()).contiguous(memory_format=torch.channels_last), wgt, bias, torch.float32, dev()).cpu()
    r64 = _ref(x, wgt, bias, torch.float64, 'cpu')
    y = _tail(x, wgt, bias).cpu()
    fin = torch.isfinite(r32)
    print(f'TAIL special {where}/{kinds}: {int((~fin).sum())} non-finite of {r32.numel()} in aten32, '
          f'{int((~torch.isfinite(y)).sum())} in HIP; NaN {int(torch.isnan(r32).sum())} / {int(torch.isnan(y).sum())}', flush=True)
    if kinds == 'finite':
        assert bool(fin.all()), 'the fp32 reference itself overflowed: the case is wrong'
        assert bool(torch.isfinite(y).all())
    else:
        assert int((~fin).sum()) > 0
    assert torch.equal(torch.isnan(y), torch.isnan(r32))
    inf32, infy = torch.isinf(r32), torch.isinf(y)
    assert torch.equal(infy, inf32) and torch.equal(y[infy], r32[inf32])        # the same Inf, sign included
    e_hip, e_ref = ref_errors(*(t[fin].numpy() for t in (y, r32, r64)))
    print(f'TAIL special {where}/{kinds}: |HIP-fp64| {e_hip:.3e}  |aten32-fp64| {e_ref:.3e} over the finite positions', flush=True)
    assert within_reference(e_hip, e_ref), (e_hip, e_ref)
    small = fin & (r64.abs() < 100.0)        # the gate above is relative to max|fp64| ~ 1.7e38: the ordinary positions on their own scale
    e_hip, e_ref = ref_errors(y[small].numpy(), r32[small].numpy(), r64[small].numpy())
    print(f'TAIL special {where}/{kinds}: |HIP-fp64| {e_hip:.3e}  |aten32-fp64| {e_ref:.3e} over the ordinary positions', flush=True)
    assert within_reference(e_hip, e_ref), (e_hip, e_ref)
    assert torch.equal(_tail(x, wgt, bias).cpu().view(torch.int32), y.view(torch.int32)), 'two calls differ'


# ----------------------------------------------------------------------------- 5. the host plan (no GPU)
def test_select_is_the_plan_and_a_declined_launch_launches_nothing():
    from op import _native
    L = _native.lib()
    sel = _native.conv3x3_tail_bf16x3_select
    for ow in range(1, 24):
        want = 16 if 9 <= ow <= 16 else 8 if 5 <= ow <= 8 else _native.FMGAN_EUNSUPPORTED
        for w in (2 * ow - 1, 2 * ow):
            assert sel(2, 16, 32, 11, w) == want, (ow, w)
    assert sel(8, 512, 512, 32, 32) == 16 and sel(8, 512, 512, 16, 16) == 8 and sel(8, 512, 512, 64, 64) == _native.FMGAN_EUNSUPPORTED
    declined = [(1, 6, 8, 16, 16), (1, 18, 8, 32, 32),                 # cin % 4 != 0
                (1, 512, 32, 70000, 32),                               # one sample's input past the 32-bit buffer range
                (1, 16, 8, 8, 8), (1, 16, 8, 34, 34)]                  # 4 wide, 17 wide
    for shape in declined:
        assert sel(*shape) == _native.FMGAN_EUNSUPPORTED, shape
        assert L.fmgan_conv3x3_tail_bf16x3_f32(None, None, None, None, *shape, SLOPE, 1, None) == _native.FMGAN_EUNSUPPORTED
    for shape in [(0, 16, 8, 16, 16), (-1, 16, 8, 16, 16), (1, 0, 8, 16, 16), (1, 16, 0, 16, 16), (1, 16, 8, 0, 16), (1, 16, 8, 16, -3)]:
        assert sel(*shape) == _native.FMGAN_EINVAL, shape
        assert L.fmgan_conv3x3_tail_bf16x3_f32(None, None, None, None, *shape, SLOPE, 1, None) == _native.FMGAN_EINVAL
    # a served shape with a NULL pointer or a bad layout flag: refused before any launch
    assert L.fmgan_conv3x3_tail_bf16x3_f32(None, None, None, None, 1, 16, 8, 16, 16, SLOPE, 1, None) == _native.FMGAN_EINVAL
    assert L.fmgan_conv3x3_tail_bf16x3_f32(None, None, None, None, 1, 16, 8, 16, 16, SLOPE, 2, None) == _native.FMGAN_EINVAL


# ----------------------------------------------------------------------------- 6. modules
def _tail_infos(b, spatial, first_x3):
    """The tail bracket's infos the routing rule gives one head on a `spatial`^2 level at batch b."""
    from psp_encoder_model.encoders import psp_encoders
    infos, s = [], spatial
    while s > 1:
        if not (first_x3 and s == spatial) and (16 if 9 <= s // 2 <= 16 else 8 if 5 <= s // 2 <= 8 else 0) in psp_encoders.TAIL_X3_WIDTHS:
            infos.append((b, 512, 512, s, s))
        s //= 2
    return infos


@gpu
def test_style_block_switch_on_vs_off_vs_fp64():
    """GradualStyleBlock(512, 512, 64) at B = 2 on a channels_last feature map: the default against FMGAN_PSP_TAIL_X3
    off (MIOpen for every convolution after the first) as the fp32 reference, both against the float64 module."""
    from psp_encoder_model.encoders import psp_encoders
    blk = psp_encoders.GradualStyleBlock(512, 512, 64)
    sd = {}
    for k, v in blk.state_dict().items():
        if k.startswith('convs'):
            sd[k] = synth.tensor('tail/blk/' + k, tuple(v.shape), scale=(2.0 / 4608) ** 0.5 if k.endswith('weight') else 0.1)
        else:
            sd[k] = synth.tensor('tail/blk/' + k, tuple(v.shape), scale=0.0 if k.endswith('bias') else 1.0)
    blk.load_state_dict(sd)
    x = synth.tensor('tail/blk/x', (2, 512, 64, 64))
    assert psp_encoders.TAIL_X3 and 16 in psp_encoders.TAIL_X3_WIDTHS, 'the narrow-tile convolutions are the default'
    with torch.no_grad():
        r64 = copy.deepcopy(blk).double()(x.double())
        g = blk.to(dev())
        xg = x.to(dev()).contiguous(memory_format=torch.channels_last)
        with launches.observed() as rec:
            on = g(xg)
            want = _tail_infos(2, 64, True)
            assert want[0] == (2, 512, 512, 32, 32) and rec.infos('conv3x3_tail_bf16x3') == want, rec.infos('conv3x3_tail_bf16x3')
            assert rec.count('conv_tail_weight_bf16x3') == len(want) and rec.count('conv_weight_bf16x3') == 1
            on2 = g(xg)
            assert rec.count('conv3x3_tail_bf16x3') == 2 * len(want)
            assert rec.count('conv_tail_weight_bf16x3') == len(want) and rec.count('conv_weight_bf16x3') == 1
            try:
                psp_encoders.TAIL_X3 = False
                off = g(xg)
            finally:
                psp_encoders.TAIL_X3 = True
            assert rec.count('conv3x3_tail_bf16x3') == 2 * len(want)
    # (on and on2 need not be the same bits: the 4-wide and smaller convolutions stay on MIOpen's split-K kernels)
    closer_to_fp64('TAIL block on', on.cpu().numpy(), off.cpu().numpy(), r64.numpy(), ref_name='MIOpen32')
    closer_to_fp64('TAIL block on (kept weight images)', on2.cpu().numpy(), off.cpu().numpy(), r64.numpy(), ref_name='MIOpen32')


@gpu
def test_encoder_routes_the_heads_by_width_class():
    """E_W_Plus at 256^2 (pyramid 16^2 / 32^2 / 64^2), 10 heads = 3 coarse, 4 middle, 3 fine, in that order: the tail
    infos are those of the rule; switched off the bracket does not appear and the latents agree within 5e-6 max|out|,
    the tolerance of the encoder goldens."""
    from psp_encoder_model.encoders import psp_encoders
    enc = psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=10))
    enc.load_state_dict(synth.state_dict('psp', enc.state_dict(), seed=7))
    enc = enc.to(dev()).eval()
    x = synth.tensor('tail/enc/x', (1, 3, 256, 256), dist='uniform').to(dev())
    with torch.no_grad(), launches.observed() as rec:
        a = enc(x)
        infos = rec.infos('conv3x3_tail_bf16x3')
        del rec.seen[:]
        try:
            psp_encoders.TAIL_X3 = False
            b = enc(x)
        finally:
            psp_encoders.TAIL_X3 = True
        assert rec.count('conv3x3_tail_bf16x3') == 0 and rec.count('conv_tail_weight_bf16x3') == 0
    want = _tail_infos(1, 16, False) * 3 + _tail_infos(1, 32, False) * 4 + _tail_infos(1, 64, True) * 3
    assert len(want) >= 7 and infos == want, infos
    d, m = float((a - b).abs().max()), float(b.abs().max())
    print(f'TAIL encoder on vs off: max|diff| {d:.3e} = {d / m:.3e} of max|out| {m:.3e}', flush=True)
    assert d <= 5e-6 * m


# ----------------------------------------------------------------------------- 7. the code object (no GPU)
def test_tail_instantiations_do_not_spill(tmp_path):
    """Two kernels, one per width class: no spilled register, no scratch, and at most 256 VGPRs — two blocks of four
    waves per CU are two waves per SIMD, half of its 512 registers each."""
    kernels = codeobj.kernel_notes(tmp_path)
    names = [k for k in kernels if 'conv3x3_tail_x3' in k]
    assert len(names) == 2 and not [n for n in names if 'conv3x3_mfma_bf16x3' in n], names
    for n in names:
        k = kernels[n]
        assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0 and k['vgpr'] <= 256, (n, k)
