"""Every tile of the fp32 modulated-conv kernel (csrc/modconv_fwd.hip, MC_TILES) at shapes that reach it — with the tile asserted.

launch_any picks the tile from the shape, the split-K plan and the fused-ToRGB flag, so a small test shape easily lands on
another tile than the one it was written for.  Here every case states the (cfg, variant, ksplit) it is meant to reach and
asserts that with _native.modconv2d_select (the launch's own planning code with the launch left out) before it runs: a change
of the dispatch fails the case instead of moving it silently.  test_every_product_tile_is_reached closes the loop against
_native.modconv2d_tiles().

Reference: the input-modulated form demod * conv(scale W, s x) in float64 on the CPU (torch), whole tensor; gate: parity.tol
against that result rounded to fp32; torch.equal where two paths must agree.  Every case prints its measured
max|HIP - fp64| / max|fp64| (profiles/modconv_tile_cases.md keeps the figures).  The largest whole float64 reference here
(the data gradient through a 259 x 257 transposed conv) takes about a second on the CPU, so no case needs output windows.

How the shapes were chosen.  A 256-position tile ('C', 'E') is launched only for >= 2 x 256 CUs blocks of 256 positions and
no split-K: 257 rows x 34 columns is 33 x 2 tiles per sample (TW = 32, 8 rows per tile: ragged in both directions, odd
height, a batch tail where the batch is odd), and a few samples / two channel tiles give the 512 blocks.  Channel counts
20 / 33 / 64 give whole 4-channel chunks, a partial last chunk (general K loop) and 16 chunks; cout 40 / 70 / 130 are ragged
against 32 / 64 / 128 (generic stores).  One case per tile has 16-byte-aligned rows (w % 4 == 0: the wide patch) and whole
channel tiles (buffer stores), as the production layers have.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from gpumem import dev, misaligned
from parity import tol as _tol

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- cases
# (b, cin, cout, h, w) -> (cfg, variant, ksplit)
E_CASES = [((8, 20, 40, 257, 34), (2, 'E', 1)),      # 5 lean chunks of 4 on the first channel tile, ragged cout on the second
           ((8, 33, 40, 257, 35), (2, 'E', 1)),      # partial last chunk, w % 4 != 0
           ((8, 16, 32, 257, 36), (2, 'E', 1))]      # aligned rows, whole channel tile
C1_CASES = [((4, 33, 70, 257, 34), (1, 'C', 1)),
            ((3, 64, 70, 257, 66), (1, 'C', 1)),     # batch tail, 16 chunks of 4
            ((2, 32, 64, 257, 258), (1, 'C', 1)),    # 9 tiles across, the last two columns wide
            ((4, 16, 64, 512, 64), (1, 'C', 1))]     # aligned rows, whole channel tile
C0_CASES = [((4, 20, 130, 257, 34), (0, 'C', 1)),
            ((4, 64, 130, 257, 34), (0, 'C', 1)),
            ((4, 32, 130, 257, 34), (0, 'C', 1)),
            ((4, 16, 128, 512, 64), (0, 'C', 1))]    # aligned rows, whole channel tile
PLAIN_CASES = E_CASES + C1_CASES + C0_CASES

# The remaining tiles of the plain and the transposed conv: (b, cin, cout, h, w, mode) -> (cfg, variant, ksplit).
# The register tiles ('A') of the plain conv serve a launch without ToRGB only where the LDS-DMA tile 'B' declines: a 1 x 1
# image packs 128 samples into a tile and the packed patches overflow the LDS image.  (The 128- and 64-channel classes
# need more than 2048 positions for that: a batch of 2049.)
OTHER_CASES = [((4, 128, 128, 64, 64, 0), (0, 'B', 4)),
               ((1, 16, 100, 49, 57, 0), (0, 'B', 1)),
               ((2049, 8, 128, 1, 1, 0), (0, 'A', 1)),
               ((3, 40, 72, 33, 33, 0), (1, 'B', 2)),
               ((2049, 12, 70, 1, 1, 0), (1, 'A', 1)),
               ((8, 32, 32, 32, 32, 0), (2, 'B', 1)),
               ((5, 12, 20, 1, 1, 0), (2, 'A', 1)),
               ((2, 24, 64, 33, 34, 1), (1, 'B', 1)),
               ((4, 128, 64, 32, 32, 1), (1, 'A', 4)),     # 'B' declines: the thin segments' patches, LDS image > 64 KB
               ((2, 64, 32, 64, 64, 1), (2, 'D', 1)),
               ((2, 33, 200, 65, 67, 1), (2, 'D', 1)),     # the 32-channel tile for a wide layer, partial last chunk
               ((3, 12, 20, 1, 1, 1), (2, 'A', 1))]

# Fused ToRGB: (b, cin, cout, h, w, keep_out) -> (cfg, variant, ksplit) of the fused launch.
RGB_CASES = [((4, 16, 20, 512, 34, True), (2, 'E', 1)),
             ((8, 16, 32, 257, 36, False), (2, 'E', 1)),
             # a 4-row image: the 256-position tile would hold two samples, the RGB epilogue reads one sample's weights per
             # block -> the launch must leave 'E' for the register tile (one sample per 128-position tile)
             ((16, 8, 32, 4, 2048, True), (2, 'A', 1)),
             ((2, 32, 32, 64, 64, True), (2, 'B', 1)),
             ((2, 16, 64, 48, 48, True), (1, 'A', 1)),
             ((1, 16, 100, 49, 57, False), (0, 'A', 1))]

# Backward roles: the kernel's own (b, cin, cout, h, w) — cin is the forward conv's Cout, the input its output gradient.
# kind 1 weights on mode 0 (data gradient of the plain conv) on the two 'C' tiles; kind 2 weights on mode 2 (data gradient
# of the transposed conv) on each stride-2 tile, with ksplit == 1 and > 1; (.., 128, .., 259, 257) run 16 chunks per block.
BWD_PLAIN_CASES = [((4, 64, 130, 257, 34), (0, 'C', 1)),
                   ((3, 64, 70, 257, 66), (1, 'C', 1))]
BWD_STRIDE2_CASES = [((2, 64, 128, 259, 257), (0, 'A', 1)),
                     ((2, 128, 128, 259, 257), (0, 'A', 1)),
                     ((2, 512, 512, 65, 65), (0, 'A', 8)),
                     ((2, 128, 64, 259, 257), (1, 'A', 1)),
                     ((2, 256, 64, 129, 131), (1, 'A', 5)),
                     ((2, 128, 40, 259, 257), (2, 'A', 1)),
                     ((1, 512, 40, 65, 67), (2, 'A', 16))]

# Tiles of the product table that no argument reaches, with the reason.  None: with the single-sample guard of the fused
# launch (see RGB_CASES) every tile is reached, the register tiles through a declined LDS-DMA tile.
UNREACHED = set()


def _select(shape, mode, rgb=False):
    from op import _native
    cfg, variant, bm, bn, ks = _native.modconv2d_select(*shape, mode, rgb=rgb)
    return (cfg, variant, ks), (bm, bn)


def _assert_tile(shape, mode, want, rgb=False):
    got, dims = _select(shape, mode, rgb)
    assert got == want, f'{shape} mode {mode} rgb {rgb}: select says {got}, this case is written for {want}'
    return f'mode {mode} cfg {got[0]} {got[1]} {dims[0]}x{dims[1]}' + (' +rgb' if rgb else ''), got[2]


# ------------------------------------------------------------------------------------------------------------ reference
def _inputs(tag, b, cin, cout, h, w):
    x = synth.tensor(f'{tag}/x', (b, cin, h, w))
    wgt = synth.tensor(f'{tag}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'{tag}/s', (b, cin), shift=1.0, scale=0.5)
    return x, wgt, s


def _dense64(u, w64, mode):
    if mode == 0:
        return F.conv2d(u, w64, padding=1)
    if mode == 1:
        return F.conv_transpose2d(u, w64.transpose(0, 1), stride=2)
    return F.conv2d(u, w64, stride=2)


def _ref64(x, wgt, s, mode):
    """demod * conv(scale W, s x) in float64."""
    cin = wgt.shape[1]
    w64 = wgt.double() * (1.0 / np.sqrt(cin * 9))
    s64 = s.double()
    demod = torch.rsqrt((w64[None] * s64[:, None, :, None, None]).square().sum((2, 3, 4)) + 1e-8)
    return _dense64(x.double() * s64[:, :, None, None], w64, mode) * demod[:, :, None, None]


def _gate(what, tile, ks, got, ref64):
    """parity.tol against the float64 result rounded to fp32; prints the measured error first."""
    g = got.cpu().numpy()
    r64 = ref64.numpy()
    r32 = r64.astype(np.float32)
    scale = float(np.abs(r64).max())
    err = float(np.abs(g.astype(np.float64) - r64).max()) / scale
    t = _tol(r32)
    print(f'TILECASE | {what} | {tile} | {ks} | {err:.2e} | {t["atol"] / scale:.2e}')
    assert np.isfinite(g).all()
    np.testing.assert_allclose(g, r32, **t)


def _chunks_per_block(cin, ks):
    chunks = (cin + 7) // 8                      # MC_KC = 8 input channels per split-K unit
    return (chunks + ks - 1) // ks


def _act64(core, noise, nw, bias):
    pre = core
    if noise is not None:
        pre = pre + float(np.float32(nw)) * noise.double()
    if bias is not None:
        pre = pre + bias.double()[None, :, None, None]
    return torch.where(pre > 0, pre, pre * float(np.float32(0.2))) * float(np.float32(2 ** 0.5))


# ------------------------------------------------------------------------------------------- the three default plain tiles
@pytest.mark.parametrize('shape,want', PLAIN_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_default_plain_tiles_vs_float64(shape, want):
    """Plain128x256DmaKc4 / Plain64x256DmaKc4 / Plain32x256DmaKc4R128: result against float64; misaligned input (4-byte patch
    pieces) and strided output give the same bits; the fused epilogue (per-sample noise, shared noise, neither noise nor
    bias) against noise + bias + LeakyReLU on the float64 core; two runs bit-identical."""
    from op import _native
    b, cin, cout, h, w = shape
    tile, ks = _assert_tile(shape, 0, want)
    x, wgt, s = _inputs(f'tiles/{shape}', *shape)
    core = _ref64(x, wgt, s, 0)
    d = dev()
    xd, wd, sd = x.to(d), wgt.to(d), s.to(d)
    scale = 1.0 / np.sqrt(cin * 9)
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    y = _native.modconv2d(xd, wt, sd, dm, 0)
    _gate(f'plain {shape}', tile, ks, y, core)
    assert torch.equal(_native.modconv2d(xd, wt, sd, dm, 0), y)                         # bit-reproducible
    xm = misaligned(xd)
    assert torch.equal(_native.modconv2d(xm, wt, sd, dm, 0), y)                         # 4-byte staging path
    buf, p0, ps, rs = _native.aligned_rows_buffer(b, cout, h, w, 1, d)
    buf.fill_(float('nan'))
    _native.modconv2d(xd, wt, sd, dm, 0, strided_out=(p0, ps, rs))
    assert torch.equal(buf[:, :, 1:1 + w].reshape(b, cout, h, w), y)
    assert torch.isnan(buf[:, :, 0]).all() and torch.isnan(buf[:, :, 1 + w:]).all()
    del buf
    bias = synth.tensor(f'tiles/{shape}/b', (cout,))
    nw = torch.tensor([0.3])
    for name, noise, bs in (('per-sample noise', synth.tensor(f'tiles/{shape}/n', (b, 1, h, w)), bias),
                            ('shared noise', synth.tensor(f'tiles/{shape}/n1', (1, 1, h, w)), bias),
                            ('no noise, no bias', None, None)):
        kw = dict(noise=None if noise is None else noise.to(d), noise_weight=None if noise is None else nw.to(d),
                  bias=None if bs is None else bs.to(d), fuse_act=True)
        ya = _native.modconv2d(xd, wt, sd, dm, 0, **kw)
        _gate(f'plain {shape} + act, {name}', tile, ks, ya, _act64(core, noise, 0.3, bs))
        assert torch.equal(_native.modconv2d(xm, wt, sd, dm, 0, **kw), ya)


# ------------------------------------------------------------------------------------------------------- the other tiles
@pytest.mark.parametrize('shape,want', OTHER_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_other_tiles_vs_float64(shape, want):
    from op import _native
    b, cin, cout, h, w, mode = shape
    tile, ks = _assert_tile(shape[:5], mode, want)
    x, wgt, s = _inputs(f'tiles/{shape}', *shape[:5])
    d = dev()
    xd, wd, sd = x.to(d), wgt.to(d), s.to(d)
    scale = 1.0 / np.sqrt(cin * 9)
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    y = _native.modconv2d(xd, wt, sd, dm, mode)
    _gate(f'mode {mode} {shape[:5]}', tile, ks, y, _ref64(x, wgt, s, mode))
    assert torch.equal(_native.modconv2d(xd, wt, sd, dm, mode), y)


# ----------------------------------------------------------------------------------------------------------- fused ToRGB
@pytest.mark.parametrize('cfg,want', RGB_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_fused_torgb_tiles_vs_two_kernel_path_and_c_oracle(cfg, want):
    """The fused-ToRGB launch on tile 'E' (and on every other tile that takes it) against the two-kernel path and the C
    oracle's to_rgb: the checks of test_conv_with_torgb_in_epilogue_vs_c_oracle, at shapes whose tile is asserted."""
    from test_hip_modconv import check_conv_with_torgb_in_epilogue
    tile, ks = _assert_tile(cfg[:5], 0, want, rgb=True)
    print(f'TILECASE | fused ToRGB {cfg[:5]} | {tile} | {ks} | (parity.tol vs the C oracle) | -')
    check_conv_with_torgb_in_epilogue(cfg)


# -------------------------------------------------------------------------------------------------------- backward roles
def _backward_role(shape, want, mode):
    """The data gradient as ModulatedConv2dFunction.backward runs it: g_u = kernel(go, weight_prep(W, kind), style = demod),
    against float64 autograd of the dense conv whose output gradient is demod * go."""
    from op import _native
    b, ck, cok, h, w = shape              # the kernel's cin = the forward conv's Cout, its cout = the forward conv's Cin
    tile, ks = _assert_tile(shape, mode, want)
    need = _native.lib().fmgan_modconv2d_workspace_bytes(b, ck, cok, h, w, mode)
    oh, ow = (h, w) if mode == 0 else ((h - 3) // 2 + 1, (w - 3) // 2 + 1)
    assert need == (ks * b * cok * oh * ow * 4 if ks > 1 else 0)
    assert _native.modconv2d_select(b, ck, cok, h, w, mode, has_workspace=False)[4] == 1
    go = synth.tensor(f'tiles/bwd/{shape}/go', (b, ck, h, w))
    wgt = synth.tensor(f'tiles/bwd/{shape}/w', (ck, cok, 3, 3))                   # forward layout [Cout, Cin, 3, 3]
    dmod = synth.tensor(f'tiles/bwd/{shape}/d', (b, ck), shift=1.0, scale=0.3)
    scale = 1.0 / np.sqrt(cok * 9)
    u = torch.zeros(b, cok, oh, ow, dtype=torch.float64, requires_grad=True)
    yf = _dense64(u, wgt.double() * scale, 0 if mode == 0 else 1)
    assert tuple(yf.shape) == (b, ck, h, w)
    ref, = torch.autograd.grad(yf, u, go.double() * dmod.double()[:, :, None, None])
    d = dev()
    wt_b = _native.modconv_weight_prep(wgt.to(d), scale, kind=1 if mode == 0 else 2)
    gu = _native.modconv2d(go.to(d), wt_b, dmod.to(d), None, mode)
    chunks = _chunks_per_block(ck, ks)
    _gate(f'data gradient, kernel shape {shape} ({chunks} chunks per block)', tile, ks, gu, ref.detach())
    assert torch.equal(_native.modconv2d(go.to(d), wt_b, dmod.to(d), None, mode), gu)
    return chunks


@pytest.mark.parametrize('shape,want', BWD_PLAIN_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_plain_data_gradient_role_on_default_tiles(shape, want):
    _backward_role(shape, want, 0)


@pytest.mark.parametrize('shape,want', BWD_STRIDE2_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_transposed_data_gradient_role_on_stride2_tiles(shape, want):
    _backward_role(shape, want, 2)


def test_stride2_cases_cover_split_and_long_k_per_tile():
    """Each stride-2 tile has a case without split-K, one with, and one whose blocks run 16 or more K chunks."""
    for cfg in (0, 1, 2):
        mine = [(sh, w) for sh, w in BWD_STRIDE2_CASES if w[0] == cfg]
        assert any(w[2] == 1 for _, w in mine) and any(w[2] > 1 for _, w in mine), cfg
        assert any(_chunks_per_block(sh[1], w[2]) >= 16 for sh, w in mine), cfg


# -------------------------------------------------------------------------------------------------------------- coverage
def test_every_product_tile_is_reached():
    """Every tile of MC_TILES is selected by some case of this file — a tile that takes fused-ToRGB launches both with and
    without one — or is listed in UNREACHED with the reason; and every case still selects what it says."""
    from op import _native
    reached = set()
    for shape, want in PLAIN_CASES + BWD_PLAIN_CASES:
        assert _select(shape, 0)[0] == want, shape
        reached.add((0, want[0], want[1], False))
    for shape, want in OTHER_CASES:
        assert _select(shape[:5], shape[5])[0] == want, shape
        reached.add((shape[5], want[0], want[1], False))
    for shape, want in BWD_STRIDE2_CASES:
        assert _select(shape, 2)[0] == want, shape
        reached.add((2, want[0], want[1], False))
    for cfg, want in RGB_CASES:
        assert _select(cfg[:5], 0, rgb=True)[0] == want, cfg
        reached.add((0, want[0], want[1], True))
    tiles = _native.modconv2d_tiles()
    assert len(tiles) == 16 and len({t[:3] for t in tiles}) == 16
    wanted = {(m, cfg, v, False) for (m, cfg, v, _bm, _bn, _rgb) in tiles} | \
             {(m, cfg, v, True) for (m, cfg, v, _bm, _bn, rgb) in tiles if rgb}
    assert reached <= wanted, sorted(reached - wanted)              # a fused launch never runs a tile that cannot take it
    assert wanted - reached == UNREACHED, sorted(wanted - reached)
    assert not (UNREACHED & reached)
