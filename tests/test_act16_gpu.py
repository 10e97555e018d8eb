"""GPU tests of the 16-bit activation path (csrc/act16.hip).  The reference of every 16-bit kernel is the
existing fp32 kernel on the widened inputs, never the new code.

Bounds.  u is the unit round-off of the storage type: 2^-8 (bf16), 2^-11 (f16).
  * bias-activation, forward and grad_input: the fp32 arithmetic is the fp32 kernel's, so y16 must EQUAL its result
    narrowed once;
  * grad_bias: the fp32 sum of the stored grad_input; exact data -> equal to the float64 sum, random data -> within
    n * 2^-24 * sum|grad_input|, the worst case of an fp32 sum of n terms;
  * FIR: integer data and dyadic taps -> every partial sum is exact -> equal to the fp32 op narrowed once; random data ->
    |y16 - y32| <= u |y32| + 2^-21 sum|k| max|x|: one rounding of the result, plus the difference of two fp32 sums of at
    most 16 products (with and without fused multiply-adds), 8 roundings of 2^-24 sum|k| max|x| each.
"""
import math

import numpy as np
import pytest
import torch

import launches
import synth
import ufd_cases
from gpumem import dev

pytestmark = pytest.mark.gpu
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SHAPES = [(1, 1, 1, 1), (2, 3, 1, 7), (2, 3, 5, 9), (1, 2, 8, 8), (3, 5, 1, 63), (1, 4, 1, 65), (2, 2, 17, 257),
          (1, 1), (3, 7), (4, 512)]
CODES = [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2)]
ALPHA, SCALE = 0.2, 2 ** 0.5


def _io(dtype):
    """The switch a dtype needs to reach the 16-bit kernels: none for bf16, activation_io('16') for f16."""
    from op import _native
    return _native.activation_io('16' if dtype == torch.float16 else 'fp32')


def _t(name, shape, dtype, **kw):
    return synth.tensor(name, shape, **kw).to(dev()).to(dtype)


def misaligned(t):
    """The same values in a view that starts one element into its storage: contiguous, 2 bytes off a 16-byte boundary."""
    store = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = store[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == t.element_size()
    return view


def _same(a, b):
    """torch.equal with NaN == NaN."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


# ------------------------------------------------------------------------------------------------- bias-activation
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dt', DTYPES)
def test_bias_act_is_the_fp32_kernel_narrowed_once(dt, shape):
    from op import _native
    dtype = DTYPES[dt]
    x = _t(f'act16/x/{shape}', shape, dtype)
    ref = _t(f'act16/ref/{shape}', shape, dtype)
    ref.view(-1)[::3] = 0                                     # the comparison `ref > 0` at its edge
    bias = synth.tensor(f'act16/b/{shape}', (shape[1],)).to(dev())      # fp32, not representable in 16 bits
    empty = x.new_empty(0)
    for variant in ('aligned', 'off by one element'):
        xs, rs = (x, ref) if variant == 'aligned' else (misaligned(x), misaligned(ref))
        for act, grad in CODES:
            for b in (bias, empty):
                for r in (rs, empty):
                    want = _native.fused_bias_act(xs.float(), b.float(), r.float(), act, grad, ALPHA, SCALE).to(dtype)
                    with _io(dtype), launches.observed() as rec:
                        got = _native.fused_bias_act(xs, b, r, act, grad, ALPHA, SCALE)
                    assert rec.infos('fused_bias_act') == [(x.numel(), 2)]
                    assert got.dtype == dtype and torch.equal(got, want), (variant, act, grad, b.numel(), r.numel())


@pytest.mark.parametrize('dt', DTYPES)
def test_bias_act_special_values(dt):
    from op import _native
    dtype = DTYPES[dt]
    fi = torch.finfo(dtype)
    vals = [float('inf'), -float('inf'), float('nan'), 0.0, -0.0, fi.max, -fi.max, fi.tiny, -fi.tiny,
            fi.smallest_normal / 4, -fi.smallest_normal / 4, fi.smallest_normal * (1 - 2.0 ** -5), 1.0, -1.0, fi.eps,
            fi.max / 2]
    x = torch.tensor(vals * 3, dtype=torch.float32, device=dev()).to(dtype).view(1, 2, 1, 24)
    ref = torch.tensor((vals[3:] + vals[:3]) * 3, dtype=torch.float32, device=dev()).to(dtype).view(1, 2, 1, 24)
    bias = torch.tensor([0.0, float(fi.tiny)], device=dev())
    for act, grad in CODES:
        for b in (bias, bias.new_empty(0)):
            want = _native.fused_bias_act(x.float(), b, ref.float(), act, grad, ALPHA, SCALE).to(dtype)
            with _io(dtype):
                got = _native.fused_bias_act(x, b, ref, act, grad, ALPHA, SCALE)
            assert _same(got, want), (act, grad, b.numel(), got, want)


def test_linear_layout_with_a_16_bit_bias_and_module_api():
    """FusedLeakyReLU converted with .bfloat16(): the bf16 bias is widened on the host (exact)."""
    from op import FusedLeakyReLU, _native
    m = FusedLeakyReLU(7).to(dev())
    with torch.no_grad():
        m.bias.copy_(synth.tensor('act16/mod/b', (7,)))
    m = m.bfloat16()
    for shape in ((3, 7), (2, 7, 5, 9)):
        x = _t(f'act16/mod/x/{shape}', shape, torch.bfloat16)
        want = _native.fused_bias_act(x.float(), m.bias.float(), x.new_empty(0).float(), 3, 0, 0.2, SCALE).bfloat16()
        got = m(x)
        assert got.dtype == torch.bfloat16 and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------- backward
def _bwd_reference(g, out, alpha, scale):
    from op import _native
    return _native.fused_bias_act(g.float(), g.new_empty(0).float(), out.float(), 3, 1, alpha, scale).to(g.dtype)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dt', DTYPES)
def test_backward_grad_input_bits_and_bias_sum(dt, shape):
    from op import _native
    dtype = DTYPES[dt]
    dims = [0] + list(range(2, len(shape)))
    n = int(np.prod(shape)) // shape[1]                       # terms per channel
    out = _t(f'act16/bwd/out/{shape}', shape, dtype)
    out.view(-1)[::5] = 0
    g_rand = _t(f'act16/bwd/g/{shape}', shape, dtype)
    g_int = torch.round(_t(f'act16/bwd/gi/{shape}', shape, torch.float32, scale=4.0)).clamp_(-8, 8).to(dtype)
    for variant in ('aligned', 'off by one element'):
        mis = (lambda t: t) if variant == 'aligned' else misaligned
        with _io(dtype):
            # exact data: scale 1, alpha 0.25, small integers -> every fp32 sum is exact
            gi, gb = _native.fused_bias_act16_backward(mis(g_int), mis(out), 0.25, 1.0)
            assert torch.equal(gi, _bwd_reference(g_int, out, 0.25, 1.0)), variant
            assert gb.dtype == torch.float32 and torch.equal(gb.double(), gi.double().sum(dims)), variant
            # random data
            gi, gb = _native.fused_bias_act16_backward(mis(g_rand), mis(out), ALPHA, SCALE)
            gi2, gb2 = _native.fused_bias_act16_backward(mis(g_rand), mis(out), ALPHA, SCALE)
        assert gi.dtype == dtype and torch.equal(gi, _bwd_reference(g_rand, out, ALPHA, SCALE)), variant
        err = (gb.double() - gi.double().sum(dims)).abs()
        bound = n * 2.0 ** -24 * gi.double().abs().sum(dims)
        print(dt, shape, variant, 'grad_bias error / bound:', float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (variant, err, bound)
        assert torch.equal(gi, gi2) and torch.equal(gb, gb2), 'not bit-reproducible'


# ------------------------------------------------------------------------------------------------- FIR
PADS = [(2, 2), (1, 1), (2, 1), (0, 0), (-1, -1), (3, 0)]
TAPS = [(1, 1), (2, 2), (4, 4), (1, 4), (4, 1)]
PLANES = [(1, 1, 1), (3, 4, 7), (2, 5, 8), (1, 9, 63), (2, 33, 65), (1, 64, 257)]


def _fir_bound(y32, k, x, dtype):
    return U[dtype] * y32.abs() + 2.0 ** -21 * float(k.abs().sum()) * float(x.float().abs().max())


@pytest.mark.parametrize('plane', PLANES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dt', DTYPES)
def test_fir_exact_and_random(dt, plane):
    from op import _native, upfirdn2d
    dtype = DTYPES[dt]
    major, h, w = plane
    x_int = torch.round(_t(f'ufd16/xi/{plane}', (1, major, h, w), torch.float32, scale=4.0)).clamp_(-8, 8).to(dtype)
    x_rand = _t(f'ufd16/xr/{plane}', (1, major, h, w), dtype)
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], device=dev())
    k44 = torch.outer(k1, k1) / 64
    ran = 0
    worst = 0.0
    for kh, kw in TAPS:
        k_exact = k44[:kh, :kw].contiguous()
        k_rand = synth.tensor(f'ufd16/k/{kh}x{kw}', (kh, kw), dist='uniform').to(dev())
        for pad in PADS:
            if h + pad[0] + pad[1] - kh + 1 <= 0 or w + pad[0] + pad[1] - kw + 1 <= 0:
                continue                                      # no output at all: refused for every dtype
            assert _native.lib().fmgan_ufd16_select(_native.dtype16_code(x_int), major, h, w, 1, kh, kw, 1, 1, 1, 1,
                                                    pad[0], pad[1], pad[0], pad[1]) == 1
            want_exact = upfirdn2d(x_int.float(), k_exact, pad=pad).to(dtype)
            y32 = upfirdn2d(x_rand.float(), k_rand, pad=pad)
            for variant in ('aligned', 'off by one element'):
                mis = (lambda t: t) if variant == 'aligned' else misaligned
                with _io(dtype), launches.observed() as rec:
                    got_exact = upfirdn2d(mis(x_int), k_exact, pad=pad)
                    got = upfirdn2d(mis(x_rand), k_rand, pad=pad)
                assert [i[-1] for i in rec.infos('upfirdn2d')] == [2, 2]
                assert got_exact.dtype == dtype and torch.equal(got_exact, want_exact), (kh, kw, pad, variant)
                err = (got.float() - y32).abs()
                bound = _fir_bound(y32, k_rand, x_rand, dtype)
                worst = max(worst, float((err / bound).max()))
                assert got.dtype == dtype and bool((err <= bound).all()), (kh, kw, pad, variant, float((err / bound).max()))
                ran += 1
    print(dt, plane, 'cases:', ran, 'worst error / bound:', worst)
    assert ran >= 2 * 6                                       # even the 1x1 plane has the 1x1 FIR at five pads + others


UP_ROWS = list(ufd_cases.UP2)                                 # the five up = 2 argument sets (generic 16-bit kernel)


@pytest.mark.parametrize('row', UP_ROWS, ids=ufd_cases.row_id)
def test_bf16_generic_kernel_up2(row):
    from op import _native
    _, major, h, w, kh, kw, up, px0, px1, py0, py1 = row
    x = _t(f'ufd16/gen/{row}', (major, h, w, 1), torch.bfloat16)
    k = synth.tensor(f'ufd16/genk/{row}', (kh, kw), dist='uniform').to(dev())
    assert _native.lib().fmgan_ufd16_select(_native.BF16, major, h, w, 1, kh, kw, up, up, 1, 1, px0, px1, py0, py1) == 0
    y32 = _native.upfirdn2d(x.float(), k, up, up, 1, 1, px0, px1, py0, py1)
    assert tuple(y32.shape[1:3]) == ufd_cases.OUT_SIZE[row]
    for xs in (x, misaligned(x)):
        got = _native.upfirdn2d(xs, k, up, up, 1, 1, px0, px1, py0, py1)
        err = (got.float() - y32).abs()
        assert got.dtype == torch.bfloat16 and bool((err <= _fir_bound(y32, k, x, torch.bfloat16)).all())


def test_bf16_generic_kernel_down2_and_minor():
    from op import _native, upfirdn2d
    x = _t('ufd16/down/x', (2, 3, 13, 18), torch.bfloat16)
    k = synth.tensor('ufd16/down/k', (4, 4), dist='uniform').to(dev())
    y32 = upfirdn2d(x.float(), k, down=2, pad=(1, 1))
    got = upfirdn2d(x, k, down=2, pad=(1, 1))
    assert got.dtype == torch.bfloat16 and bool(((got.float() - y32).abs() <= _fir_bound(y32, k, x, torch.bfloat16)).all())
    xm = _t('ufd16/minor/x', (2, 6, 7, 3), torch.bfloat16)                     # minor = 3: generic kernel at up = down = 1
    y32 = _native.upfirdn2d(xm.float(), k, 1, 1, 1, 1, 2, 1, 1, 2)
    got = _native.upfirdn2d(xm, k, 1, 1, 1, 1, 2, 1, 1, 2)
    assert bool(((got.float() - y32).abs() <= _fir_bound(y32, k, xm, torch.bfloat16)).all())


# ------------------------------------------------------------------------------------------------- autograd
def test_fused_leaky_relu_gradients_to_second_order():
    """Each differentiation is one bias-activation call: grad_input and the second-order term are one rounding away from
    the fp32 Function on the widened tensors; grad_bias is an fp32 sum of the rounded grad_input."""
    from op import fused_leaky_relu
    dtype, u = torch.bfloat16, U[torch.bfloat16]
    shape = (2, 3, 5, 9)
    n = 2 * 5 * 9
    x16 = _t('act16/ag/x', shape, dtype).requires_grad_(True)
    go16 = _t('act16/ag/go', shape, dtype).requires_grad_(True)
    ggi16 = _t('act16/ag/ggi', shape, dtype)
    b = synth.tensor('act16/ag/b', (3,)).to(dev()).requires_grad_(True)
    ggbias = synth.tensor('act16/ag/ggb', (3,)).to(dev())
    res = {}
    for name, (x, go, ggi) in dict(lo=(x16, go16, ggi16), hi=tuple(
            t.detach().float().requires_grad_(t.requires_grad) for t in (x16, go16, ggi16))).items():
        y = fused_leaky_relu(x, b)
        gi, gb = torch.autograd.grad(y, (x, b), go, create_graph=True)
        gg, = torch.autograd.grad(gi, go, ggi, retain_graph=True)
        ggb, = torch.autograd.grad((gi, gb), go, (ggi, ggbias))      # the double backward with a non-zero bias term
        res[name] = (y, gi, gb, gg, ggb)
    (y, gi, gb, gg, ggb), (y32, gi32, gb32, gg32, ggb32) = res['lo'], res['hi']
    assert y.dtype == gi.dtype == gg.dtype == ggb.dtype == dtype and gb.dtype == b.dtype == torch.float32
    assert torch.equal(y, y32.to(dtype)) and torch.equal(gi, gi32.to(dtype)) and torch.equal(gg, gg32.to(dtype))
    assert torch.equal(ggb, ggb32.to(dtype)) and not torch.equal(ggb, gg)
    bound = u * gi32.abs().sum((0, 2, 3)) + n * 2.0 ** -24 * gi32.abs().sum((0, 2, 3)) * 2
    assert bool(((gb - gb32).abs() <= bound).all()), (gb, gb32, bound)


def test_upfirdn2d_gradients_to_second_order():
    from op import upfirdn2d
    dtype = torch.bfloat16
    k = synth.tensor('ufd16/ag/k', (4, 4), dist='uniform').to(dev())
    x16 = _t('ufd16/ag/x', (2, 3, 9, 17), dtype).requires_grad_(True)
    for pad in ((2, 2), (1, 1)):
        y16 = upfirdn2d(x16, k, pad=pad)
        go16 = _t(f'ufd16/ag/go/{pad}', y16.shape, dtype).requires_grad_(True)
        ggi16 = _t(f'ufd16/ag/ggi/{pad}', x16.shape, dtype)
        gi16, = torch.autograd.grad(y16, x16, go16, create_graph=True)
        gg16, = torch.autograd.grad(gi16, go16, ggi16)
        x, go, ggi = x16.detach().float().requires_grad_(True), go16.detach().float().requires_grad_(True), ggi16.float()
        y = upfirdn2d(x, k, pad=pad)
        gi, = torch.autograd.grad(y, x, go, create_graph=True)
        gg, = torch.autograd.grad(gi, go, ggi)
        for got, want, src in ((y16, y, x16), (gi16, gi, go16), (gg16, gg, ggi16)):
            assert got.dtype == dtype and got.shape == want.shape
            assert bool(((got.float() - want).abs() <= _fir_bound(want.detach(), k, src.detach(), dtype)).all()), pad


# ------------------------------------------------------------------------------------------------- routing
def test_routing_under_autocast_and_the_switch():
    import stylegan2
    from op import FusedLeakyReLU, _native, upfirdn2d
    act = FusedLeakyReLU(4).to(dev())
    blur = stylegan2.Blur([1, 3, 3, 1], pad=(2, 2)).to(dev())
    x = _t('act16/route/x', (2, 4, 16, 16), torch.bfloat16)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        with _native.activation_io('16'), launches.observed() as rec:
            y, z = act(x), blur(x)
        assert y.dtype == z.dtype == torch.bfloat16
        assert rec.infos('fused_bias_act') == [(x.numel(), 2)] and [i[-1] for i in rec.infos('upfirdn2d')] == [2]
        with _native.activation_io('16'), launches.observed() as rec:            # an fp32 input stays on the fp32 kernels
            y32 = act(x.float())
        assert y32.dtype == torch.float32 and rec.infos('fused_bias_act') == [(x.numel(), 4)]
        with launches.observed() as rec:                                          # 'fp32' mode: exactly as before
            yf, zf = act(x), blur(x)
        assert yf.dtype == zf.dtype == torch.float32
        assert rec.infos('fused_bias_act') == [(x.numel(), 4)] and [i[-1] for i in rec.infos('upfirdn2d')] == [4]
    assert torch.equal(y, yf.bfloat16()) and torch.equal(y32, yf)
    # f16 outside the switch: today's route, the generic kernels, the same bits
    xh = x.half()
    k = blur.kernel
    assert torch.equal(upfirdn2d(xh, k, pad=(2, 2)).view(-1),
                       _native.upfirdn2d(xh.reshape(-1, 16, 16, 1), k, 1, 1, 1, 1, 2, 2, 2, 2, force_path=0).view(-1))
    bh = act.bias.detach().half()
    want = torch.empty_like(xh)
    st = _native.lib().fmgan_fused_bias_act(_native.F16, xh.data_ptr(), bh.data_ptr(), None, want.data_ptr(), xh.numel(), 4,
                                            256, 3, 0, 0.2, SCALE, torch.cuda.current_stream().cuda_stream)
    assert st == 0 and torch.equal(_native.fused_bias_act(xh, bh, xh.new_empty(0), 3, 0, 0.2, SCALE), want)
    # wrong device / CPU operands raise
    with pytest.raises(RuntimeError):
        _native.fused_bias_act16(x, torch.zeros(4), None, 3, 0, 0.2, 1.0)
    with pytest.raises(RuntimeError):
        _native.upfirdn2d16(x.reshape(-1, 16, 16, 1), k.cpu(), 1, 1, 1, 1, 2, 2, 2, 2)
    with pytest.raises(RuntimeError):
        _native.fused_bias_act16(x.view(torch.int16), None, None, 3, 0, 0.2, 1.0)


# ------------------------------------------------------------------------------------------------- Discriminator
def _d_quantities(D, img, mode):
    """(logits, d logits.sum / d img, R1 penalty) of D on img: 'fp32', or under autocast with activation_io(mode)."""
    import contextlib
    from op import _native
    from Util.training_util import d_r1_loss
    img = img.detach().clone().requires_grad_(True)
    with contextlib.ExitStack() as st:
        if mode != 'fp32':
            st.enter_context(torch.autocast('cuda', dtype=torch.bfloat16))
            st.enter_context(_native.activation_io('16' if mode == '16' else 'fp32'))
        logits = D(img)
        r1 = d_r1_loss(logits, img)
        grad, = torch.autograd.grad(logits.float().sum(), img, retain_graph=True)
        D.zero_grad(set_to_none=True)
        r1.backward()                                         # the double backward of the R1 step
        gw = torch.cat([p.grad.detach().float().flatten() for p in D.parameters() if p.grad is not None])
    D.zero_grad(set_to_none=True)
    return [t.detach().float() for t in (logits, grad, r1.reshape(1), gw)]


@pytest.fixture(scope='module')
def d_runs():
    import stylegan2
    from nets import load
    D = load(stylegan2.Discriminator(64), 'discriminator', 8, eval=False)
    img = synth.tensor('act16/d/img', (4, 3, 64, 64), dist='uniform').to(dev())
    with launches.observed() as rec:
        lo = _d_quantities(D, img, '16')
    sizes16 = {i[-1] for i in rec.infos('fused_bias_act')} | {i[-1] for i in rec.infos('upfirdn2d')}
    return dict(D=D, img=img, fp32=_d_quantities(D, img, 'fp32'), glue=_d_quantities(D, img, 'fp32 glue'), lo=lo,
                sizes16=sizes16)


def test_discriminator_under_autocast_with_16_bit_activations(d_runs):
    """Gate: err('16') <= 4 err('fp32' mode) + u max|fp32 result| for the logits, the input gradient, the R1 penalty and
    the parameter gradients of the R1 penalty; err(.) is the largest deviation from the fp32 run.  The fp32-glue autocast
    run is the existing behaviour and sets the scale; 4x is this project's margin over a reference's own error."""
    u = U[torch.bfloat16]
    assert d_runs['sizes16'] == {2}, d_runs['sizes16']        # every activation / blur launch of the run was 16-bit
    for name, ref, glue, lo in zip(('logits', 'input gradient', 'r1', 'r1 parameter gradients'), d_runs['fp32'],
                                   d_runs['glue'], d_runs['lo']):
        assert bool(torch.isfinite(lo).all()), name
        e_glue, e_lo = float((glue - ref).abs().max()), float((lo - ref).abs().max())
        gate = 4 * e_glue + u * float(ref.abs().max())
        print(f'{name}: err(fp32 mode) {e_glue:.4g}  err(16) {e_lo:.4g}  gate {gate:.4g}  max|fp32| {float(ref.abs().max()):.4g}')
        assert e_lo <= gate, (name, e_lo, gate)


def test_converted_discriminator_runs(d_runs):
    import copy
    from Util.training_util import d_r1_loss
    D = copy.deepcopy(d_runs['D']).bfloat16()
    img = d_runs['img'].bfloat16().requires_grad_(True)
    with launches.observed() as rec:
        logits = D(img)
        r1 = d_r1_loss(logits, img)
        (logits.sum() + r1).backward()                        # first-order and R1 double backward in one pass
    assert logits.dtype == torch.bfloat16 and bool(torch.isfinite(logits.float()).all())
    assert bool(torch.isfinite(r1.float()).all())
    assert {i[-1] for i in rec.infos('fused_bias_act')} | {i[-1] for i in rec.infos('upfirdn2d')} == {2}
    for name, p in D.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.bfloat16 and bool(torch.isfinite(p.grad.float()).all()), name


# ------------------------------------------------------------------------------------------------- Trainer
TRAIN_B = 2


def _trainer_nets():
    """The smallest networks the training tests build (tests/cases.py TRAIN_STEP_CASE), with tests/synth.py's weights."""
    import cases
    import stylegan2
    from nets import encoders, load
    size = cases.TRAIN_STEP_CASE['size']
    e_tsr, e_w, e_wp = encoders(int(math.log2(size)) * 2 - 2)
    return dict(G=load(stylegan2.Generator(size, 512, 2), 'generator', 4), E_Tsr=e_tsr, E_W=e_w, E_W_Plus=e_wp,
                D=load(stylegan2.Discriminator(size), 'discriminator', 8))


def _trainer_args(**over):
    import cases
    import train_3_encoder as T
    hp = cases.TRAIN_HP
    args = T.default_args(tsr_encode='Photo Image', lr=hp['lr'], r1=hp['r1'], d_reg_every=hp['d_reg_every'],
                          g_reg_every=hp['g_reg_every'], generator_path_reg_weight=hp['path_reg_weight'],
                          path_reg_batch_shrink=hp['path_reg_batch_shrink'], l1_loss_lambda=hp['l1_loss_lambda'],
                          ema_fuse=True)
    for k, v in over.items():
        setattr(args, k, v)
    return args


def _train_iteration(tr, it):
    """Iteration `it` on its own fixed batch, the generator's noise seeded and the path-length sample fixed."""
    import cases
    size = cases.TRAIN_STEP_CASE['size']
    torch.manual_seed(100 + it)
    photo = synth.tensor(f'act16/train/{it}/photo', (TRAIN_B, 3, 256, 256), dist='uniform').to(dev())
    render = synth.tensor(f'act16/train/{it}/render', (TRAIN_B, 3, 256, 256), dist='uniform').to(dev())
    ref = synth.tensor(f'act16/train/{it}/ref', (TRAIN_B, 3, size, size), dist='uniform').to(dev())
    tr.step(photo, render, ref, ppl_choice=[1])


@pytest.fixture(scope='module')
def trainer_runs():
    import copy
    import train_3_encoder as T
    out = {}
    nets = _trainer_nets()                                    # built once; every run trains its own copy
    for name, over, iters in (('fp32', {}, 1), ('off', dict(precision='bf16', bf16_io=False), 2),
                              ('on', dict(precision='bf16', bf16_io=True), 2)):
        tr = T.Trainer(copy.deepcopy(nets), _trainer_args(**over), dev())
        losses, sizes = [], set()
        for it in range(iters):
            with launches.observed() as rec:
                _train_iteration(tr, it)
            losses.append({k: float(v.detach()) for k, v in tr.loss_dict.items()})
            sizes |= {i[-1] for i in rec.infos('fused_bias_act')} | {i[-1] for i in rec.infos('upfirdn2d')}
        out[name] = dict(tr=tr, losses=losses, sizes=sizes)
    return out


def test_trainer_in_bf16_with_and_without_16_bit_activations(trainer_runs):
    u = U[torch.bfloat16]
    assert trainer_runs['fp32']['sizes'] == {4} and trainer_runs['off']['sizes'] == {4}
    assert 2 in trainer_runs['on']['sizes']
    for name in ('off', 'on'):
        run = trainer_runs[name]
        tr = run['tr']
        for it, ld in enumerate(run['losses']):
            assert ld and all(math.isfinite(v) for v in ld.values()), (name, it, ld)
        for net in list(tr.bare.values()) + [tr.g_ema]:
            assert all(p.dtype == torch.float32 for p in net.parameters())
        for opt in (tr.g_enc_optim, tr.d_optim, tr.d_edit_optim):
            if opt is None:
                continue
            for st in opt.state.values():
                assert st['exp_avg'].dtype == st['exp_avg_sq'].dtype == torch.float32
        assert tr.ema_plan is not None and tr.ema_plan.rebuilds == 1          # the fused EMA still accepts the pair
    d32, d_off, d_on = (trainer_runs[k]['losses'][0]['d'] for k in ('fp32', 'off', 'on'))
    gate = 4 * abs(d_off - d32) + u * abs(d32)
    print(f'd loss, first iteration: fp32 {d32:.6g}  bf16 {d_off:.6g}  bf16 + 16-bit activations {d_on:.6g}  gate {gate:.4g}')
    assert abs(d_on - d32) <= gate
