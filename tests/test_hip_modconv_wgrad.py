"""Every weight-gradient kernel of csrc/modconv_wgrad.hip, on every path its launch can take, against float64 on the CPU.

The launch picks between a 32 x 32-tile kernel (modconv_wgrad_f32: plain conv with fewer than 48 channels on one side; pixel
tiles 16 or 32 wide) and three 64 x 64-tile kernels (modconv_wgrad64_f32<log2 TW, SP>: <5,1> and <4,1> for the plain conv,
<4,2> for the transposed and the stride-2 conv), each of the latter with a vector staging path (rows of whole 16-byte groups
from a 16-byte-aligned tensor) and a guarded scalar one.  Which of them a shape reaches is asked of the library
(_native.modconv_wgrad_select: the launch's own plan function with the launch left out) and asserted before the launch, so a
case cannot quietly drift onto another kernel; the workspace the launch is given is sized by the same plan
(ksplit * 9 * cout * cin floats).

Reference: the float64 weight gradient of the dense conv of (style * x, demod * go) on the CPU — mode 0
torch.nn.grad.conv2d_weight, modes 1 and 2 autograd through conv_transpose2d / conv2d(stride 2) of a zero weight.  Bound:
atol 2e-5 * max|ref|, rtol 2e-5, the bound tests/test_hip_modconv.py holds these kernels to; a second call gives the same
bits (fixed-order split over pixels)."""
import pytest
import torch
import torch.nn.functional as F

import launches
import synth
from gpumem import dev, misaligned

pytestmark = pytest.mark.gpu

SCALE = 0.37


def _out_size(mode, h, w):
    """Size of go for a conv input of h x w."""
    if mode == 1:
        return 2 * h + 1, 2 * w + 1
    if mode == 2:
        return (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return h, w


def _inputs(case):
    """(go, demod, x, style) on the CPU, drawn as in test_wgrad_kernel_vs_fp64 / test_strided_wgrad_kernel_vs_fp64."""
    mode, b, cin, cout, h, w = case
    oh, ow = _out_size(mode, h, w)
    tag = f'wgk/{case}'
    go = synth.tensor(tag + '/go', (b, cout, max(oh, 1), max(ow, 1)))     # (a declined shape may have no output at all)
    x = synth.tensor(tag + '/x', (b, cin, h, w))
    s = synth.tensor(tag + '/s', (b, cin), shift=1.0, scale=0.5)
    d = synth.tensor(tag + '/d', (b, cout), shift=1.0, scale=0.3)
    return go, d, x, s


def _reference(mode, go, d, x, s):
    """float64, CPU: SCALE * weight gradient of the dense conv of u = s * x with output gradient g = d * go."""
    cout, cin = go.shape[1], x.shape[1]
    u = x.double() * s.double()[:, :, None, None]
    g = go.double() if d is None else go.double() * d.double()[:, :, None, None]
    if mode == 0:
        return torch.nn.grad.conv2d_weight(u, (cout, cin, 3, 3), g, padding=1) * SCALE
    wref = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(u, wref.transpose(0, 1), stride=2) if mode == 1 else F.conv2d(u, wref, stride=2)
    ref, = torch.autograd.grad(y, wref, g)
    return ref * SCALE


def _workspace_bytes(case):
    from op import _native
    mode, b, cin, cout, h, w = case
    return _native.lib().fmgan_modconv_wgrad_mode_workspace_bytes(b, cin, cout, h, w, mode)


def _select(case, aligned16=True):
    from op import _native
    mode, b, cin, cout, h, w = case
    return _native.modconv_wgrad_select(b, cin, cout, h, w, mode, aligned16=aligned16)


def check_wgrad(case, expect, demod=True, loop=None, misalign=()):
    """The one body of this file.  case = (mode, b, cin, cout, h, w) with h, w the conv input's size; expect = (family, TW,
    SP, vec) as modconv_wgrad_select must answer for 16-byte-aligned tensors; loop: a predicate on (ksplit, tiles_per_split,
    ntiles) where the case is about the tile loop; misalign: names of the operands ('go', 'x') to run once more as views one
    float into a larger buffer — the scalar staging path by alignment, which must give the aligned run's bits."""
    from op import _native
    mode, b, cin, cout, h, w = case
    family, tw, sp, ks, tps, ntiles, vec = _select(case)
    print(f'wgrad {case} demod={demod}: family {family} TW {tw} SP {sp} vec {vec} ksplit {ks} tiles/split {tps} ntiles {ntiles}')
    assert (family, tw, sp, vec) == expect
    assert _workspace_bytes(case) == ks * 9 * cout * cin * 4 > 0
    assert ks == -(-ntiles // tps)
    if loop is not None:
        assert loop(ks, tps, ntiles), (ks, tps, ntiles)
    go, d, x, s = _inputs(case)
    if not demod:
        d = None
    ref = _reference(mode, go, d, x, s)
    god, xd, sd = go.to(dev()), x.to(dev()), s.to(dev())
    dd = d.to(dev()) if demod else None
    assert god.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == 0
    with launches.observed() as obs:
        gw = _native.modconv_wgrad(god, dd, xd, sd, SCALE, mode=mode)
    assert obs.seen == [('modconv_wgrad', (b, cin, cout, h, w, mode))]
    assert gw is not None and tuple(gw.shape) == (cout, cin, 3, 3)
    peak = float(ref.abs().max())
    err = float((gw.cpu().double() - ref).abs().max())
    print(f'wgrad {case}: max error {err:.3e} = {err / peak:.3e} of max|ref| {peak:.3e}')
    torch.testing.assert_close(gw.cpu().double(), ref, atol=2e-5 * peak, rtol=2e-5)
    assert torch.equal(gw, _native.modconv_wgrad(god, dd, xd, sd, SCALE, mode=mode))      # bit-reproducible
    if misalign:
        unshifted = 'x' if mode == 1 else 'go'                # operand A of the 64 x 64 kernels: its alignment decides `vec`
        assert unshifted in misalign
        assert _select(case, aligned16=False) == (family, tw, sp, ks, tps, ntiles, False)
        gom = misaligned(god) if 'go' in misalign else god
        xm = misaligned(xd) if 'x' in misalign else xd
        for name, t in (('go', gom), ('x', xm)):
            assert t.is_contiguous() and (t.data_ptr() % 16 != 0) == (name in misalign) and t.data_ptr() % 4 == 0
        assert torch.equal(_native.modconv_wgrad(gom, dd, xm, sd, SCALE, mode=mode), gw)
    return gw


def _case(case, expect, **kw):
    ident = 'm{}_b{}_{}to{}_{}x{}'.format(*case) + ''.join(f'_{k}' for k in kw)
    return pytest.param(case, expect, kw, id=ident)


# ------------------------------------------------------------------ the 32 x 32-tile kernel (mode 0, one side < 48 channels)
@pytest.mark.parametrize('case,expect,kw', [
    _case((0, 2, 20, 40, 9, 16), (32, 16, 1, False)),              # TW 16, ragged cin and cout, two o tiles, batch 2
    _case((0, 2, 20, 40, 9, 16), (32, 16, 1, False), demod=False),
    _case((0, 1, 3, 33, 5, 21), (32, 16, 1, False)),               # TW 16, ragged width (second x tile 5 wide), cin = 3
    _case((0, 3, 47, 47, 7, 33), (32, 32, 1, False)),              # TW 32, ragged everything, 2 x 2 channel tiles
    _case((0, 1, 64, 32, 8, 32), (32, 32, 1, False)),              # the wide side >= 48, still the 32-tile kernel
    _case((0, 1, 32, 64, 8, 32), (32, 32, 1, False)),
])
def test_wgrad32_kernel_vs_fp64_cpu(case, expect, kw):
    check_wgrad(case, expect, **kw)


def test_wgrad32_kernel_second_trip_of_the_tile_loop_vs_fp64_cpu():
    """tiles_per_split >= 2: the block stages a second pixel tile into the LDS it has just read, behind the barrier at the top
    of the loop.  (0, 2, 512, 40, 64, 64) has 64 pixel tiles for 32 channel-tile pairs: two tiles per block on the 256 compute
    units of an MI355X.  The split grows with the chip, so the batch is raised until the plan says two."""
    batch = next((b for b in range(2, 9) if _select((0, b, 512, 40, 64, 64))[4] >= 2), None)
    assert batch is not None, 'no batch up to 8 gives this chip two tiles per block'
    case = (0, batch, 512, 40, 64, 64)
    print('shape used:', case)
    check_wgrad(case, (32, 32, 1, False), loop=lambda ks, tps, ntiles: tps >= 2 and ks >= 2)


# ------------------------------------------------------------------ the 64 x 64-tile kernels
@pytest.mark.parametrize('case,expect,kw', [
    # <5,1>: plain conv, rows of 32 pixels and more
    _case((0, 1, 48, 48, 4, 32), (64, 32, 1, True), demod=False),
    _case((0, 1, 48, 48, 1, 32), (64, 32, 1, True), loop=lambda ks, tps, n: (ks, n) == (1, 1)),    # h = 1: no second tile row
    # one block walks both samples: the scales of sample 1 are fetched while sample 0 is on the matrix pipe
    _case((0, 2, 48, 48, 4, 32), (64, 32, 1, True), loop=lambda ks, tps, n: ks == 1 and tps == n == 4),
    _case((0, 1, 64, 64, 4, 33), (64, 32, 1, False)),                                              # scalar staging by width
    # <4,1>: plain conv, rows of 16 .. 31 pixels
    _case((0, 1, 48, 48, 2, 16), (64, 16, 1, True), loop=lambda ks, tps, n: (ks, n) == (1, 1)),    # a single tile
    _case((0, 2, 50, 70, 5, 18), (64, 16, 1, False)),
    _case((0, 1, 64, 64, 3, 31), (64, 16, 1, False)),
    _case((0, 1, 64, 64, 4, 16), (64, 16, 1, True), misalign=('go', 'x')),
    # <4,2>, transposed conv (operand A is x)
    _case((1, 1, 48, 48, 2, 16), (64, 16, 2, True), loop=lambda ks, tps, n: (ks, n) == (1, 1)),
    _case((1, 2, 48, 64, 5, 17), (64, 16, 2, False)),
    _case((1, 1, 64, 48, 3, 18), (64, 16, 2, False)),
    _case((1, 1, 48, 48, 2, 16), (64, 16, 2, True), demod=False),
    _case((1, 1, 64, 64, 4, 16), (64, 16, 2, True), misalign=('x',)),
    # <4,2>, stride-2 conv (operand A is go, (h - 3) / 2 + 1 rows of (w - 3) / 2 + 1)
    _case((2, 1, 48, 48, 5, 33), (64, 16, 2, True), loop=lambda ks, tps, n: (ks, n) == (1, 1)),    # go 2 x 16
    _case((2, 1, 64, 50, 6, 36), (64, 16, 2, False)),          # go 2 x 17; the last row and column of the even-sized x unused
    _case((2, 2, 48, 48, 4, 34), (64, 16, 2, True)),           # go 1 x 16
    _case((2, 2, 48, 48, 4, 34), (64, 16, 2, True), demod=False),
])
def test_wgrad64_kernels_vs_fp64_cpu(case, expect, kw):
    check_wgrad(case, expect, **kw)


def test_wgrad64_kernel_uneven_last_split_vs_fp64_cpu():
    """A last split shorter than the others (ntiles % tiles_per_split != 0): its block leaves the tile loop early, and the
    finish kernel still adds one slab per split.  (0, 1, 64, 64, 18, 32) has 9 pixel tiles, at least 4 per block: 5 + 4.  The
    height is raised until the plan says so."""
    h = next((h for h in range(18, 40) if _select((0, 1, 64, 64, h, 32))[5] % _select((0, 1, 64, 64, h, 32))[4]), None)
    assert h is not None
    case = (0, 1, 64, 64, h, 32)
    print('shape used:', case)
    check_wgrad(case, (64, 32, 1, True), loop=lambda ks, tps, ntiles: ks >= 2 and ntiles % tps != 0)


# ------------------------------------------------------------------ shapes the library declines
@pytest.mark.parametrize('case', [
    (0, 1, 64, 64, 4, 15), (0, 1, 20, 40, 4, 15),        # mode 0, w = 15, at both channel classes
    (1, 1, 64, 64, 4, 15),                               # mode 1, w = 15
    (2, 1, 64, 64, 9, 32),                               # mode 2, w = 32: go is 15 wide
    (2, 1, 64, 64, 2, 40),                               # mode 2, h = 2: no output row
    (1, 1, 64, 47, 4, 16), (2, 1, 64, 47, 9, 40),        # cout = 47: below the 64 x 64 tile, which modes 1 and 2 need
    (1, 1, 47, 64, 4, 16), (2, 1, 47, 64, 9, 40),        # cin = 47
], ids=lambda c: 'm{}_b{}_{}to{}_{}x{}'.format(*c))
def test_wgrad_declined_shapes_launch_nothing(case):
    """The wrapper returns None without opening a launch bracket, select says family 0, the workspace query says 0 bytes, and
    the C entry point itself, handed real tensors and a real workspace, returns FMGAN_EUNSUPPORTED and leaves gw untouched."""
    from op import _native
    mode, b, cin, cout, h, w = case
    assert _select(case) == (0, 0, 0, 0, 0, 0, False) == _select(case, aligned16=False)
    assert _workspace_bytes(case) == 0
    go, d, x, s = (t.to(dev()) for t in _inputs(case))
    with launches.observed() as obs:
        assert _native.modconv_wgrad(go, d, x, s, SCALE, mode=mode) is None
        assert _native.modconv_wgrad(go, d, x, s, SCALE, fast_only=True, mode=mode) is None
    assert obs.seen == []
    gw = torch.full((cout, cin, 3, 3), float('nan'), device=dev())
    ws = torch.zeros(4 * 9 * cout * cin, device=dev())
    stream = torch.cuda.current_stream().cuda_stream
    st = _native.lib().fmgan_modconv_wgrad_mode_f32(go.data_ptr(), d.data_ptr(), x.data_ptr(), s.data_ptr(), gw.data_ptr(),
                                                    b, cin, cout, h, w, mode, SCALE, ws.data_ptr(), ws.numel() * 4, stream)
    assert st == _native.FMGAN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(gw).all() and not ws.any()
