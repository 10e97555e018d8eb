"""GPU tests of the two reduced-cost modulated convs (csrc/modconv_bf16.hip: fmgan_modconv2d_bf16, fmgan_modconv2d_bf16x3)
at their edges: special values, the smallest grids the predicate admits, the shapes just outside it, a seeded sweep, and
the first-order data gradient under modconv_precision('bf16').

Every reference is a float64 convolution on the CPU, never the kernel under test:
  * bf16   — oracle/torch_oracle.py::modconv_bf16_reference (both operands rounded to bf16, exact products, wide
             accumulator), at 2e-5 of max|ref|: fp32 summation error only;
  * bf16x3 — the float64 convolution of the UNROUNDED operands, under the rule of test_bf16x3_kernel_has_fp32_accuracy:
             its error at most 2 x the fp32 kernel's on the same inputs + 2e-6, both relative to max|ref|.
Which kernel ran is read from the launch brackets (tests/launches.py), not inferred from an error."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from gpumem import dev
from launches import observed
from modconv_bf16_cases import inputs as _inputs

pytestmark = pytest.mark.gpu

BRACKET = {'f32': 'modconv2d', 'bf16': 'modconv2d_bf16', 'bf16x3': 'modconv2d_bf16x3'}


# ----------------------------------------------------------------------------- shared pieces
def _conv64(u, wq, mode):
    if mode == 0:
        return F.conv2d(u, wq, padding=1)
    if mode == 1:
        return F.conv_transpose2d(u, wq.transpose(0, 1), stride=2)
    return F.conv2d(u, wq, stride=2)


def _ref64(x, wgt, s, dm, mode, scale):
    """float64 convolution of the unrounded fp32 operands fl32(x*style), fl32(scale*W)."""
    u = (x.float() * s.float()[:, :, None, None]).double()
    wq = (wgt.float() * torch.tensor(scale, dtype=torch.float32)).double()
    ref = _conv64(u, wq, mode)
    return ref if dm is None else ref * dm.cpu().double()[:, :, None, None]


def _modconv_launches(rec):
    return [(n, i) for n, i in rec.seen if n.startswith('modconv2d')]


def _launch(xd, wt, sd, dm, mode, precision, bracket=None, ambient=False):
    """One modconv2d under the recorder: exactly one modconv2d* bracket was opened, `bracket` (default: the precision's
    own kernel), with this launch's (b, cin, cout, h, w, mode).  ambient: the precision comes from the context manager."""
    from op import _native
    b, cin, h, w = xd.shape
    with observed() as rec:
        if ambient:
            with _native.modconv_precision(precision):
                y = _native.modconv2d(xd, wt, sd, dm, mode)
        else:
            y = _native.modconv2d(xd, wt, sd, dm, mode, precision=precision)
    seen = _modconv_launches(rec)
    assert seen == [(bracket or BRACKET[precision], (b, cin, wt.shape[2], h, w, mode))], seen
    return y


def _device_operands(x, wgt, s, scale, demod):
    from op import _native
    xd, wd, sd = x.to(dev()), wgt.to(dev()), s.to(dev())
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale) if demod else None
    return xd, wt, sd, dm


def _x3_rule(y3, y32, ref, sel, what):
    """e3 <= 2 * e32 + 2e-6 over the positions `sel`, both errors relative to that subset's max|ref|."""
    assert int(sel.sum()) > 0, what
    r = ref[sel]
    mx = float(r.abs().max())
    e3 = float((y3[sel].double() - r).abs().max()) / mx
    e32 = float((y32[sel].double() - r).abs().max()) / mx
    print(f'BFE x3 {what}: |x3-fp64| {e3:.3e}  |f32-fp64| {e32:.3e}  of max|ref| {mx:.4g}', flush=True)
    assert e3 <= 2 * e32 + 2e-6, (what, e3, e32)


def _bf16_rule(y, ref, sel, what):
    """|y - ref| <= 2e-5 * max|ref| over the positions `sel` (the max over the same subset)."""
    assert int(sel.sum()) > 0, what
    r = ref[sel]
    mx = float(r.abs().max())
    err = float((y[sel].double() - r).abs().max())
    print(f'BFE bf16 {what}: |bf16-def| {err / mx:.3e} of max|ref| {mx:.4g}', flush=True)
    assert err <= 2e-5 * mx, (what, err / mx)


def _check_bf16(x, wgt, s, scale, mode, demod, what):
    from op import _native
    from oracle import torch_oracle as T
    b, cin, h, w = x.shape
    assert _native.lib().fmgan_modconv2d_bf16_supported(b, cin, wgt.shape[0], h, w, mode) == 1, what
    xd, wt, sd, dm = _device_operands(x, wgt, s, scale, demod)
    y = _launch(xd, wt, sd, dm, mode, 'bf16').cpu()
    ref = T.modconv_bf16_reference(x, wgt, s, None if dm is None else dm.cpu(), mode, scale)
    assert y.shape == ref.shape, what
    _bf16_rule(y, ref, torch.ones_like(ref, dtype=torch.bool), what)
    return y


def _check_x3(x, wgt, s, scale, mode, demod, what):
    from op import _native
    b, cin, h, w = x.shape
    assert _native.lib().fmgan_modconv2d_bf16x3_supported(b, cin, wgt.shape[0], h, w, mode) == 1, what
    xd, wt, sd, dm = _device_operands(x, wgt, s, scale, demod)
    y3 = _launch(xd, wt, sd, dm, mode, 'bf16x3').cpu()
    y32 = _launch(xd, wt, sd, dm, mode, 'f32').cpu()
    ref = _ref64(x, wgt, s, dm, mode, scale)
    assert y3.shape == ref.shape, what
    _x3_rule(y3, y32, ref, torch.ones_like(ref, dtype=torch.bool), what)
    return y3


# ----------------------------------------------------------------------------- A. special values
FINITE = [0.0, -0.0, 3.3e38, -3.3e38, 3.4e38, -3.4e38, 1e-38, -1e-38, 1e-39, 1e-40]
NONFINITE = [float('inf'), -float('inf'), float('nan')]
# 32 -> 32 channels: two K chunks, the second through the register prefetch.  Input sizes: mode 0 two tile rows and two
# tile columns of the x3 tile (8 x 32), mode 1 the minimum grid, mode 2 (bf16 only) a ragged 5 x 33 grid.
SP_HW = {0: (12, 40), 1: (4, 32), 2: (11, 67)}


def _place(mode, k):
    """Input position of value k (it also has channel k to itself).  Columns 3 apart in mode 0 (a 3 x 3 window spans 3),
    2 apart in mode 1 (an output reads 2 x 2 inputs), 5 apart in mode 2: no output reads two placed values."""
    h, w = SP_HW[mode]
    if mode == 0:
        return (5 * k) % h, 3 * k
    if mode == 1:
        return k % h, 2 * k + 3
    return (4 * k) % h, 5 * k


def _special_case(where, kinds, mode):
    """(x, wgt, style, plain x, touched): every ordinary operand uniform in [-0.5, 0.5], scale 1, style all ones, no
    demodulation, so the placed values reach the rounding / the split unchanged.  'input': value k at channel k,
    _place(mode, k).  'weight': value k at W[k, k % cin, 1, 1], the centre tap (mode 0: never meets the padding; mode 1:
    owns the (odd, odd) output phase alone).  touched [oh, ow]: the outputs whose window holds a placed input."""
    values = FINITE + (NONFINITE if kinds == 'all' else [])
    h, w = SP_HW[mode]
    tag = f'bfe/sp/{where}/{mode}'
    x = synth.tensor(tag + '/x', (1, 32, h, w), dist='uniform', scale=0.5)
    wgt = synth.tensor(tag + '/w', (32, 32, 3, 3), dist='uniform', scale=0.5)
    assert float(x.abs().max()) <= 0.5 and float(wgt.abs().max()) <= 0.5 and float(x.abs().min()) > 0
    plain = x.clone()
    placed = torch.zeros(1, 1, h, w, dtype=torch.float64)
    for k, v in enumerate(values):
        if where == 'input':
            py, px = _place(mode, k)
            x[0, k, py, px] = v
            placed[0, 0, py, px] += 1
        else:
            wgt[k, k % 32, 1, 1] = v
    per_window = _conv64(placed, torch.ones(1, 1, 3, 3, dtype=torch.float64), mode)[0, 0]
    assert float(per_window.max()) <= 1, 'two placed values in one window: the case is wrong'
    return x, wgt, torch.ones(1, 32), plain, per_window > 0


def _finite_case_is_sound(kinds, ref64):
    if kinds == 'finite':
        assert bool(torch.isfinite(ref64).all()) and float(ref64.abs().max()) < 3.4e38, \
            'the float64 reference itself is not finite below 3.4e38: the case is wrong'
    else:
        assert int((~torch.isfinite(ref64)).sum()) > 0, 'no non-finite output in the reference: the case is wrong'


def _isolation(precision, y, plain, wgt, s, mode, touched):
    """The outputs whose window holds none of the placed inputs are bit-equal to the launch on the plain input."""
    xd, wt, sd, _ = _device_operands(plain, wgt, s, 1.0, False)
    y0 = _launch(xd, wt, sd, None, mode, precision).cpu()
    assert torch.isfinite(y0).all()
    clean = ~touched
    assert int(clean.sum()) > 0 and int(touched.sum()) > 0
    assert torch.equal(y[0][:, clean].view(torch.int32), y0[0][:, clean].view(torch.int32))


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('where', ['input', 'weight'])
@pytest.mark.parametrize('kinds', ['finite', 'all'])
def test_bf16x3_special_values(where, kinds, mode):
    """'finite': +-0, +-3.3e38, +-3.4e38 (beyond the largest bf16: its RNE rounding is Inf) and the 1e-38 .. 1e-40
    neighbourhood give a finite output of fp32 accuracy, on the ordinary positions (|ref| < 100) at their own scale as
    well as over all positions.  'all' adds +-Inf and NaN: the output is non-finite exactly where the float64
    convolution is, and accurate elsewhere; which non-finite value appears is not asserted (the modulated kernel has no
    fp32 recomputation of such tiles)."""
    x, wgt, s, plain, touched = _special_case(where, kinds, mode)
    ref = _ref64(x, wgt, s, None, mode, 1.0)
    _finite_case_is_sound(kinds, ref)
    xd, wt, sd, _ = _device_operands(x, wgt, s, 1.0, False)
    y3 = _launch(xd, wt, sd, None, mode, 'bf16x3').cpu()
    y32 = _launch(xd, wt, sd, None, mode, 'f32').cpu()
    fin = torch.isfinite(ref)
    print(f'BFE x3 special {where}/{kinds}/m{mode}: non-finite {int((~fin).sum())} of {ref.numel()} in fp64, '
          f'{int((~torch.isfinite(y3)).sum())} in bf16x3 (NaN {int(torch.isnan(y3).sum())}), '
          f'{int((~torch.isfinite(y32)).sum())} in f32', flush=True)
    if kinds == 'finite':
        assert bool(torch.isfinite(y3).all()), f'{int((~torch.isfinite(y3)).sum())} non-finite outputs of finite operands'
    assert torch.equal(torch.isfinite(y3), fin)
    what = f'special {where}/{kinds}/m{mode}'
    _x3_rule(y3, y32, ref, fin & (ref.abs() < 100.0), what + ' ordinary positions')
    _x3_rule(y3, y32, ref, fin, what + ' finite positions')
    if where == 'input':
        _isolation('bf16x3', y3, plain, wgt, s, mode, touched)


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('where', ['input', 'weight'])
@pytest.mark.parametrize('kinds', ['finite', 'all'])
def test_bf16_special_values(where, kinds, mode):
    """The bf16 kernel against its definition, in which a value beyond the largest bf16 (+-3.4e38) IS +-Inf: NaN where the
    definition has NaN, Inf of the same sign where it has Inf, and the 2e-5 bound on the finite positions — over the
    ordinary ones (|ref| < 100) at their own scale and over the whole finite set."""
    from oracle import torch_oracle as T
    x, wgt, s, plain, touched = _special_case(where, kinds, mode)
    _finite_case_is_sound(kinds, _ref64(x, wgt, s, None, mode, 1.0))
    ref = T.modconv_bf16_reference(x, wgt, s, None, mode, 1.0)
    xd, wt, sd, _ = _device_operands(x, wgt, s, 1.0, False)
    y = _launch(xd, wt, sd, None, mode, 'bf16').cpu()
    inf_r, inf_y = torch.isinf(ref), torch.isinf(y)
    print(f'BFE bf16 special {where}/{kinds}/m{mode}: NaN {int(torch.isnan(ref).sum())} / {int(torch.isnan(y).sum())}, '
          f'Inf {int(inf_r.sum())} / {int(inf_y.sum())} (definition / kernel) of {ref.numel()}', flush=True)
    assert int(inf_r.sum()) > 0                                  # 3.4e38 rounds to Inf in every case
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    assert torch.equal(inf_y, inf_r) and torch.equal(y[inf_y].double(), ref[inf_r])          # the same Inf, sign included
    fin = torch.isfinite(ref)
    what = f'special {where}/{kinds}/m{mode}'
    _bf16_rule(y, ref, fin & (ref.abs() < 100.0), what + ' ordinary positions')
    _bf16_rule(y, ref, fin, what + ' finite positions')
    if where == 'input':
        _isolation('bf16', y, plain, wgt, s, mode, touched)


# ----------------------------------------------------------------------------- C. shape edges
# (b, cin, cout, h, w, mode).  The minimum position grid is 4 x 32: in mode 1 that is a 5 x 33 quad grid, one complete
# tile plus ragged ones in both directions; in mode 2 a 9 x 65 or 10 x 66 input.
MIN_GRIDS = [(1, 16, 32, 4, 32, 0), (2, 32, 64, 4, 32, 0), (1, 16, 32, 4, 32, 1), (1, 32, 64, 4, 32, 1)]
MIN_GRIDS_MODE2 = [(1, 16, 32, 9, 65, 2), (1, 16, 64, 10, 66, 2)]
EVEN_MODE2 = (2, 32, 96, 12, 68, 2)


@pytest.mark.parametrize('demod', [True, False])
@pytest.mark.parametrize('cfg', MIN_GRIDS + MIN_GRIDS_MODE2 + [EVEN_MODE2])
def test_bf16_minimum_grids(cfg, demod):
    x, wgt, s, scale = _inputs(cfg)
    y = _check_bf16(x, wgt, s, scale, cfg[5], demod, f'{cfg} demod {demod}')
    if cfg == EVEN_MODE2:
        # a stride-2 valid conv never reads the last row and column of an even-sized input
        x[:, :, -1, :] = float('nan')
        x[:, :, :, -1] = float('nan')
        xd, wt, sd, dm = _device_operands(x, wgt, s, scale, demod)
        y_nan = _launch(xd, wt, sd, dm, 2, 'bf16').cpu()
        assert torch.equal(y_nan.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize('demod', [True, False])
@pytest.mark.parametrize('cfg', MIN_GRIDS)
def test_bf16x3_minimum_grids(cfg, demod):
    x, wgt, s, scale = _inputs(cfg)
    _check_x3(x, wgt, s, scale, cfg[5], demod, f'{cfg} demod {demod}')


OUTSIDE = [
    # (cfg, the predicates that must say 0)
    ((1, 32, 32, 8, 31, 0), ('bf16', 'bf16x3')),          # w = 31
    ((1, 32, 32, 3, 40, 0), ('bf16', 'bf16x3')),          # h = 3
    ((1, 32, 32, 11, 64, 2), ('bf16', 'bf16x3')),         # mode 2 at w = 64: gw = 31
    ((1, 24, 32, 8, 40, 0), ('bf16', 'bf16x3')),          # cin = 24
    ((1, 32, 48, 8, 40, 0), ('bf16', 'bf16x3')),          # cout = 48
    ((1, 32, 32, 11, 67, 2), ('bf16x3',)),                # mode 2 is served by bf16 only
]


@pytest.mark.parametrize('cfg,unserved', OUTSIDE)
def test_just_outside_the_predicate_runs_the_fp32_kernel(cfg, unserved):
    from op import _native
    b, cin, cout, h, w, mode = cfg
    x, wgt, s, scale = _inputs(cfg)
    xd, wt, sd, dm = _device_operands(x, wgt, s, scale, True)
    y32 = _launch(xd, wt, sd, dm, mode, 'f32')
    for precision in unserved:
        assert getattr(_native.lib(), f'fmgan_modconv2d_{precision}_supported')(b, cin, cout, h, w, mode) == 0, (cfg, precision)
        y = _launch(xd, wt, sd, dm, mode, precision, bracket='modconv2d', ambient=True)
        assert torch.equal(y.view(torch.int32), y32.view(torch.int32)), (cfg, precision)
    if unserved == ('bf16x3',):
        assert _native.lib().fmgan_modconv2d_bf16_supported(b, cin, cout, h, w, mode) == 1


def _sweep_case(rng, n, modes):
    mode = modes[n % len(modes)]
    b = int(rng.integers(1, 4))
    cin = int(rng.choice([16, 32, 48, 80]))
    cout = int(rng.choice([32, 64, 96, 160]))
    h, w = int(rng.integers(4, 21)), int(rng.integers(32, 76))
    if mode == 2:       # (h, w) drawn above is the position grid; the input that gives it, odd or even
        h, w = 2 * h + 1 + int(rng.integers(0, 2)), 2 * w + 1 + int(rng.integers(0, 2))
    x = torch.from_numpy(rng.standard_normal((b, cin, h, w)).astype(np.float32))
    wgt = torch.from_numpy(rng.standard_normal((cout, cin, 3, 3)).astype(np.float32))
    s = torch.from_numpy((1.0 + 0.5 * rng.standard_normal((b, cin))).astype(np.float32))
    return mode, x, wgt, s, float(np.float32(1.0 / np.sqrt(cin * 9))), bool(n % 4)


def test_bf16_random_shapes_vs_its_definition():
    """Seeded sweep, the three modes in turn, after test_modconv_random_shapes_vs_c_oracle."""
    rng = np.random.default_rng(47)
    for n in range(12):
        mode, x, wgt, s, scale, demod = _sweep_case(rng, n, (0, 1, 2))
        _check_bf16(x, wgt, s, scale, mode, demod, f'mode {mode} b{x.shape[0]} {x.shape[1]}->{wgt.shape[0]} '
                                                   f'{x.shape[2]}x{x.shape[3]} demod {demod}')


def test_bf16x3_random_shapes_vs_fp64():
    rng = np.random.default_rng(53)
    for n in range(12):
        mode, x, wgt, s, scale, demod = _sweep_case(rng, n, (0, 1))
        _check_x3(x, wgt, s, scale, mode, demod, f'mode {mode} b{x.shape[0]} {x.shape[1]}->{wgt.shape[0]} '
                                                 f'{x.shape[2]}x{x.shape[3]} demod {demod}')


# ----------------------------------------------------------------------------- D. first-order backward under 'bf16'
# (mode, b, cin, cout, h, w): forward and data gradient both served (mode 1's data gradient is mode 2 on a
# (2h+1) x (2w+1) input); UNSERVED's swapped cout is 48, no multiple of 32: its data gradient stays on the fp32 kernel.
BWD = [(0, 2, 32, 64, 8, 32), (0, 1, 64, 32, 12, 40), (1, 2, 32, 32, 4, 32), (1, 1, 64, 96, 9, 33)]
UNSERVED = (0, 2, 48, 64, 8, 32)


def _bwd_operands(case):
    mode, b, cin, cout, h, w = case
    oh, ow = (2 * h + 1, 2 * w + 1) if mode == 1 else (h, w)
    x = synth.tensor(f'bfe/bw/{case}/x', (b, cin, h, w))
    wgt = synth.tensor(f'bfe/bw/{case}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'bfe/bw/{case}/s', (b, cin), shift=1.0, scale=0.5)
    go = synth.tensor(f'bfe/bw/{case}/go', (b, cout, oh, ow))
    return x, wgt, s, go, float(np.float32(1.0 / np.sqrt(cin * 9)))


def _infos(case):
    """(forward info, data-gradient info with the roles of cin and cout swapped)."""
    mode, b, cin, cout, h, w = case
    return (b, cin, cout, h, w, mode), ((b, cout, cin, h, w, 0) if mode == 0 else (b, cout, cin, 2 * h + 1, 2 * w + 1, 2))


def _backward(case, demod, precision):
    """modulated_conv2d + backward(go), both inside the precision block.  -> (gx, gw, gs, the modconv2d* launches)."""
    from op import _native
    from op.modconv import modulated_conv2d
    x, wgt, s, go, scale = _bwd_operands(case)
    xd, wd, sd = (t.to(dev()).requires_grad_(True) for t in (x, wgt, s))
    with _native.modconv_precision(precision):
        wt = _native.modconv_weight_prep(wd.detach(), scale)
        with observed() as rec:
            y = modulated_conv2d(xd, wd, sd, wt, demod, case[0], scale)
            y.backward(go.to(dev()))
            torch.cuda.synchronize()
    return xd.grad.cpu(), wd.grad.cpu(), sd.grad.cpu(), _modconv_launches(rec)


def _close(got, ref, what):
    ref = ref.numpy()
    np.testing.assert_allclose(got.numpy(), ref, atol=2e-4 * float(np.abs(ref).max()), rtol=2e-4, err_msg=what)


def _gu_reference(case, demod, rounded):
    from op import _native
    from oracle import torch_oracle as T
    x, wgt, s, go, scale = _bwd_operands(case)
    d = _native.modconv_demod(wgt.to(dev()), s.to(dev()), scale).cpu() if demod else None
    return T.modconv_bf16_dgrad_reference(go, wgt, d, case[0], scale, x.shape[2:], rounded=rounded)


@pytest.mark.parametrize('demod', [True, False])
@pytest.mark.parametrize('case', BWD + [UNSERVED])
def test_bf16_first_order_backward(case, demod, monkeypatch):
    """loss.backward() under modconv_precision('bf16'): the data gradient runs on the bf16 kernel with the swapped-role
    weight layouts (kind 1 in mode 0, kind 2 and mode 2 for the transposed conv) and the demodulation riding as the
    style.  gx and (without demodulation) gs against the float64 adjoint of the forward definition applied to
    bf16(go * d); the weight gradient never runs on bf16: bit-equal to the 'f32' call without demodulation.  With
    demodulation the d-terms of gs and gw read the bf16 forward output: within the per-layer bf16 bound (1e-2 of the
    max) of the 'f32' gradients."""
    served = case != UNSERVED
    x, wgt, s, go, scale = _bwd_operands(case)
    # Below 48 channels on a side, and for the transposed conv, the weight gradient is MIOpen's, whose default fp32
    # algorithm is not bit-reproducible from one call to the next (profiles/r02_determinism.md; on the two batch-2,
    # 32-channel shapes here 13835 of 18432 and 5124 of 9216 elements differed between two 'f32' calls): its
    # deterministic algorithm is asked for, so that the bit-equality below compares the two precisions and not two
    # summation orders.
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)          # restored after the test
    gx, gw, gs, seen = _backward(case, demod, 'bf16')
    gx32, gw32, gs32, seen32 = _backward(case, demod, 'f32')
    fwd, dgrad = _infos(case)
    assert seen == [('modconv2d_bf16', fwd), ('modconv2d_bf16' if served else 'modconv2d', dgrad)], seen
    gu = _gu_reference(case, demod, rounded=served)
    _close(gx, gu * s.double()[:, :, None, None], f'gx {case} demod {demod}')
    assert seen32 == [('modconv2d', fwd), ('modconv2d', dgrad)], seen32
    if not demod:
        _close(gs, (gu * x.double()).sum((2, 3)), f'gs {case}')
        assert torch.equal(gw.view(torch.int32), gw32.view(torch.int32))
    else:
        for name, g, g32 in (('gs', gs, gs32), ('gw', gw, gw32)):
            dist = float((g - g32).abs().max() / g32.abs().max())
            print(f'BFE bwd {case} demod: |{name}(bf16) - {name}(f32)| / max = {dist:.3e}', flush=True)
            assert dist < 1e-2, (name, case, dist)


@pytest.mark.parametrize('case', BWD)
def test_bf16_backward_with_create_graph(case):
    """torch.autograd.grad(..., create_graph=True) under 'bf16': the composite's DenseConv / DenseConvDgrad reach the
    bf16 kernel too — the same gx, every contraction on modconv2d_bf16."""
    from op import _native
    from op.modconv import modulated_conv2d
    x, wgt, s, go, scale = _bwd_operands(case)
    xd = x.to(dev()).requires_grad_(True)
    wd, sd = wgt.to(dev()), s.to(dev())
    with _native.modconv_precision('bf16'):
        wt = _native.modconv_weight_prep(wd, scale)
        with observed() as rec:
            y = modulated_conv2d(xd, wd, sd, wt, True, case[0], scale)
            gx, = torch.autograd.grad(y, xd, go.to(dev()), create_graph=True)
            torch.cuda.synchronize()
    # the forward, then the composite's own forward (DenseConv) and its adjoint (DenseConvDgrad): the graph-keeping path
    fwd, dgrad = _infos(case)
    seen = _modconv_launches(rec)
    assert seen == [('modconv2d_bf16', fwd), ('modconv2d_bf16', fwd), ('modconv2d_bf16', dgrad)], seen
    gu = _gu_reference(case, True, rounded=True)
    _close(gx.detach().cpu(), gu * s.double()[:, :, None, None], f'gx {case} create_graph')
