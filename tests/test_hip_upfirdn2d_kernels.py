"""Every fast kernel of csrc/upfirdn2d.hip (register row-march, LDS-DMA ring, plane-tile, up=2 polyphase) at arguments that
reach it — with the kernel asserted, and with pads that differ between x and y.

plan_ufd picks the kernel from the arguments, so a small test shape easily lands on the generic kernel instead of the one it
was written for, and the Python op has one pad pair for both axes, so tests that mirror it cannot tell pad_x0 from pad_y0.
Here every case (tests/ufd_cases.py) first asserts with fmgan_upfirdn2d_select — the launch's own plan with the launch left
out — that its kernel is the one that runs; the ring is chosen by address, so its cases insist on path 5 and a refusal fails.

Reference: oracle.c_oracle.upfirdn2d on the float64 copies of input and taps (the plain loop over the reference's own
steps).  Gate: the project's per-op fp32 tolerance scaled by the output's magnitude, atol = 1e-5 * max(1, |ref|max),
rtol = 1e-5, as test_hip_ops.py::test_upfirdn2d_random_arguments_vs_c_oracle.  Inputs and taps are standard normal
(synth.tensor, cases.make_fir(('rand', kh, kw, seed))).  Bit equality is asserted only where include/fmgan_hip.h promises
it: the ring against the register row-march, a strided read against the contiguous one, and the fused blur against the
generic kernel followed by fmgan_noise_bias_act_f32.
"""
import numpy as np
import pytest
import torch

import cases
import synth
from gpumem import dev
import ufd_cases as U

pytestmark = pytest.mark.gpu
F32 = 0


def _tol(ref_max):
    return dict(atol=1e-5 * max(1.0, float(ref_max)), rtol=1e-5)


def _select(row, major=None):
    from op import _native
    kernel, mj, in_h, in_w, kh, kw, up, px0, px1, py0, py1 = row
    return _native.lib().fmgan_upfirdn2d_select(F32, mj if major is None else major, in_h, in_w, 1, kh, kw, up, up, 1, 1,
                                                px0, px1, py0, py1)


def _assert_kernel(row, major=None):
    """select names the row's kernel (1 for a ring row: no addresses in this query) and the table's out size holds."""
    from op import _native
    kernel, _, in_h, in_w, kh, kw, up, px0, px1, py0, py1 = row
    sel = _select(row, major)
    want = 1 if kernel == 5 else kernel
    assert sel == want, f'{U.row_id(row)}: select says {sel}, this case is written for kernel {want}'
    out = _native.upfirdn2d_out_size(in_h, in_w, kh, kw, up, up, 1, 1, px0, px1, py0, py1)
    assert out == U.OUT_SIZE[row]
    return out


def _inputs(row, major=None):
    """(x [major, in_h, in_w] f32, taps [kh, kw] f32) on the CPU; the tap seed is the row's place in the tables."""
    kernel, mj, in_h, in_w, kh, kw = row[:6]
    mj = mj if major is None else major
    x = synth.tensor(f'ufdk/{U.row_id(row)}/x', (mj, in_h, in_w))
    k = cases.make_fir(('rand', kh, kw, 100 + U.ALL_ROWS.index(row)))
    return x, k


def _oracle(x, k, row):
    """float64 oracle of planes x [n, in_h, in_w] -> [n, out_h, out_w]."""
    from oracle import c_oracle
    up, px0, px1, py0, py1 = row[6:]
    n, h, w = x.shape
    ref = c_oracle.upfirdn2d(x.double().numpy().reshape(n, h, w, 1), k.double().numpy(), (up, up), (1, 1),
                             (px0, px1, py0, py1))
    assert ref.dtype == np.float64
    return ref[..., 0]


def _check(y, ref, what):
    y = y.detach().cpu().numpy().reshape(ref.shape)
    err = float(np.abs(y - ref).max())
    print(f'{what}: max|hip - f64| = {err:.3e}, |f64|max = {float(np.abs(ref).max()):.3e}')
    np.testing.assert_allclose(y, ref, err_msg=what, **_tol(np.abs(ref).max()))


def _run(x, k, row, force_path=-1):
    """The contiguous entry point with the row's four pads; x [n, in_h, in_w] on the GPU -> [n, out_h, out_w]."""
    from op import _native
    up, px0, px1, py0, py1 = row[6:]
    n, h, w = x.shape
    y = _native.upfirdn2d(x.reshape(n, h, w, 1), k, up, up, 1, 1, px0, px1, py0, py1, force_path)
    return y.view(n, y.shape[1], y.shape[2])


def _aligned(x, px0):
    """x [n, h, w] (GPU) in the aligned-row layout for pad_x0 = px0, NaN everywhere outside the image:
    (storage, pointer of element (0, 0, 0), plane stride, row stride)."""
    from op import _native
    n, h, w = x.shape
    buf, p0, ps, rs = _native.aligned_rows_buffer(n, 1, h, w, px0, x.device)
    buf.fill_(float('nan'))
    off = px0 % 4
    buf[:, :, off:off + w] = x
    assert p0 == buf.data_ptr() + 4 * off and rs >= off + w
    return buf, p0, ps, rs


def _strided(p0, ps, rs, x, k, row, force_path=-1):
    from op import _native
    px0, px1, py0, py1 = row[7:]
    n, h, w = x.shape
    return _native.upfirdn2d_strided(p0, x.device, n, h, w, ps, rs, k, px0, px1, py0, py1, force_path=force_path)


# ----------------------------------------------------------------------------------------------------------- row-march
@pytest.mark.parametrize('row', U.ROWMARCH, ids=U.row_id)
def test_rowmarch_directed(row):
    """ufd_rowmarch_f32<1 | 2 | 4> at its edges: ragged strips and row tiles, crops, windows beside the image, the narrowest
    and the shortest plane it takes, 1..4 taps per axis."""
    oh, ow = _assert_kernel(row)
    x, k = _inputs(row)
    ref = _oracle(x, k, row)
    assert ref.shape[1:] == (oh, ow)
    y = _run(x.to(dev()), k.to(dev()), row)
    _check(y, ref, U.row_id(row))
    # and the same planes read through row / plane strides (the kernel's lo / hi bounds and row pointer arithmetic)
    xd = x.to(dev())
    buf, p0, ps, rs = _aligned(xd, row[7])
    ys = _strided(p0, ps, rs, xd, k.to(dev()), row, force_path=4)
    assert not torch.isnan(ys).any()
    _check(ys, ref, U.row_id(row) + ' strided')


def test_rowmarch_tall_tiles():
    """[16 * CUs, 65, 65] -> [., 64, 64]: the grid is large enough for 32-row tiles, so a wave runs the march loop 8 times
    (every other row-march case in this file stops after one pass of 4 rows).  Whole tensor against the generic kernel,
    three planes against the oracle."""
    row = U.ROWMARCH_TALL
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    major = U.rowmarch_tall_major(cus)
    assert major * 1 * 2 >= 32 * cus > major * 1 * 1         # strips = 1; 32-row tiles pass the threshold, 64-row tiles do not
    if cus == 256:
        assert major == row[1]
    _assert_kernel(row, major)
    x, k = _inputs(row, major)
    xd, kd = x.to(dev()), k.to(dev())
    y = _run(xd, kd, row)
    y0 = _run(xd, kd, row, force_path=0)
    t = _tol(y0.abs().max())
    bad = (y - y0).abs() > t['atol'] + t['rtol'] * y0.abs()
    assert not bool(bad.any()), f'{int(bad.sum())} elements differ from the generic kernel, first plane {int(bad.nonzero()[0, 0])}'
    sample = [0, 1, major - 1]
    ref = _oracle(x[sample], k, row)
    _check(y[sample], ref, U.row_id(row))


# ---------------------------------------------------------------------------------------------------------------- ring
@pytest.mark.parametrize('row', U.RING, ids=U.row_id)
def test_ring_directed(row):
    """ufd_dmaring_f32 with unequal pads, 2..4 taps per axis and a partial last row tile, against the register row-march on
    the same aligned-row buffer (equal bits) and the oracle; the NaN that fills the buffer's padding must not leak."""
    _assert_kernel(row)
    x, k = _inputs(row)
    ref = _oracle(x, k, row)
    xd, kd = x.to(dev()), k.to(dev())
    buf, p0, ps, rs = _aligned(xd, row[7])
    ring = _strided(p0, ps, rs, xd, kd, row, force_path=5)      # an `unsupported` RuntimeError here fails the case
    regs = _strided(p0, ps, rs, xd, kd, row, force_path=4)
    assert not torch.isnan(ring).any() and not torch.isnan(regs).any()
    assert torch.equal(ring, regs)
    _check(ring, ref, U.row_id(row) + ' ring')
    _check(regs, ref, U.row_id(row) + ' row-march')


def test_ring_refuses_negative_pad_x0():
    """pad_x0 = -1 puts the first tap column left of the aligned position 0: path 5 must refuse, the automatic launch runs
    the register row-march."""
    row = U.RING_REFUSED
    _assert_kernel(row)
    x, k = _inputs(row)
    ref = _oracle(x, k, row)
    xd, kd = x.to(dev()), k.to(dev())
    buf, p0, ps, rs = _aligned(xd, row[7])
    with pytest.raises(RuntimeError, match='unsupported'):
        _strided(p0, ps, rs, xd, kd, row, force_path=5)
    y = _strided(p0, ps, rs, xd, kd, row)
    assert not torch.isnan(y).any()
    _check(y, ref, U.row_id(row))


# ---------------------------------------------------------------------------------------------------------- plane-tile
@pytest.mark.parametrize('row', U.PLANETILE, ids=U.row_id)
def test_planetile_directed(row):
    """ufd_planetile_f32: 1 x 1 planes, crops, a wide plane of one output row, the largest plane it takes (48 KB of LDS), 64
    planes per block with a ragged last block, and windows that are almost all padding."""
    oh, ow = _assert_kernel(row)
    x, k = _inputs(row)
    ref = _oracle(x, k, row)
    assert ref.shape[1:] == (oh, ow)
    y = _run(x.to(dev()), k.to(dev()), row)
    _check(y, ref, U.row_id(row))


def test_planetile_bound_is_exclusive_above():
    """One row past the 12288-element bound the plan must answer the generic kernel (a plane-tile launch would ask for more
    LDS than a block may have), and that kernel serves the shape."""
    row = U.PLANETILE_OVER
    assert row[2] * row[3] == 12291
    _assert_kernel(row)
    x, k = _inputs(row)
    y = _run(x.to(dev()), k.to(dev()), row)
    _check(y, _oracle(x, k, row), U.row_id(row))


def test_planetile_strided_read():
    """The plane-tile kernel's strided copy (aligned-row intermediate) with unequal pads: equal bits to the contiguous read,
    NaN padding must not leak."""
    row = U.PLANETILE_STRIDED
    _assert_kernel(row)
    x, k = _inputs(row)
    xd, kd = x.to(dev()), k.to(dev())
    yc = _run(xd, kd, row)
    buf, p0, ps, rs = _aligned(xd, row[7])
    ys = _strided(p0, ps, rs, xd, kd, row)
    assert torch.equal(ys, yc)
    _check(ys, _oracle(x, k, row), U.row_id(row))


# ----------------------------------------------------------------------------------------------------------------- up2
@pytest.mark.parametrize('row', U.UP2, ids=U.row_id)
def test_up2_directed(row):
    """ufd_up2_f32<PY, PX> for the pad parities that symmetric pads never give (<0,1>, <1,0>), rows narrower than one vector
    load, every out_w % 4 store tail, odd out_h, 1..4 taps per axis."""
    oh, ow = _assert_kernel(row)
    x, k = _inputs(row)
    ref = _oracle(x, k, row)
    assert ref.shape[1:] == (oh, ow)
    y = _run(x.to(dev()), k.to(dev()), row)
    _check(y, ref, U.row_id(row))


def test_up2_second_grid_trip():
    """[CUs / 16 + 1, 512, 512] -> [., 1024, 1024]: more 2 x 4 output blocks than 32 * CUs * 256 threads, so the grid-stride
    loop of ufd_up2_f32 takes a second trip, as the production ToRGB skip upsample does.  Whole tensor against the generic
    kernel, first and last plane (the last one is written by the second trip) against the oracle."""
    row = U.UP2_TRIP
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    major = U.up2_trip_major(cus)
    assert major * 256 * 512 > 32 * cus * 256 >= (major - 1) * 256 * 512
    if cus == 256:
        assert major == row[1]
    _assert_kernel(row, major)
    x, k = _inputs(row, major)
    xd, kd = x.to(dev()), k.to(dev())
    y = _run(xd, kd, row)
    y0 = _run(xd, kd, row, force_path=0)
    t = _tol(y0.abs().max())
    bad = (y - y0).abs() > t['atol'] + t['rtol'] * y0.abs()
    assert not bool(bad.any()), f'{int(bad.sum())} elements differ from the generic kernel, first plane {int(bad.nonzero()[0, 0])}'
    sample = [0, major - 1]
    _check(y[sample], _oracle(x[sample], k, row), U.row_id(row))


# ------------------------------------------------------------------------------------------- fused epilogue, unequal pads
def _fused_blur(p0, device, b, c, in_h, in_w, ps, rs, k, pads, nz, nw, bias, alpha, scale, force_path=-1):
    """fmgan_blur_noise_bias_act_path_f32 with four pads (op/_native/activation.py::blur_noise_bias_act has one pair, as its caller);
    a refusal raises."""
    from op import _native
    kh, kw = k.shape
    px0, px1, py0, py1 = pads
    oh, ow = _native.upfirdn2d_out_size(in_h, in_w, kh, kw, 1, 1, 1, 1, px0, px1, py0, py1)
    out = torch.full((b, c, oh, ow), float('nan'), dtype=torch.float32, device=device)
    with _native.on_device(out) as stream:
        st = _native.lib().fmgan_blur_noise_bias_act_path_f32(
            p0, _native.fp(k), _native.fp(out), b, c, in_h, in_w, ps, rs, kh, kw, px0, px1, py0, py1, _native.fp(nz),
            _native.fp(nw), _native.fp(bias), 1 if nz is None else nz.shape[0], float(alpha), float(scale), force_path,
            stream)
    _native.check(st, 'blur_noise_bias_act')
    return out


@pytest.mark.parametrize('row', U.FUSED, ids=U.row_id)
def test_fused_blur_unequal_pads(row):
    """fmgan_blur_noise_bias_act_f32 with pad_x != pad_y on each of its three kernels (ring, row-march, plane-tile): equal
    bits to the generic kernel followed by fmgan_noise_bias_act_f32, with per-sample and with shared noise, with and
    without bias.  The row's planes are taken once as `major` samples of one channel (per-sample noise indexes them) and
    once as one sample of `major` channels (the bias does)."""
    from op import _native
    kernel, major, in_h, in_w, kh, kw, up, px0, px1, py0, py1 = row
    oh, ow = _assert_kernel(row)
    x, k = _inputs(row)
    xd, kd = x.to(dev()), k.contiguous().to(dev())
    buf, p0, ps, rs = _aligned(xd, px0)
    y2 = _strided(p0, ps, rs, xd, kd, row, force_path=0)
    assert not torch.isnan(y2).any()
    _check(y2, _oracle(x, k, row), U.row_id(row) + ' generic, strided')
    nw = torch.tensor([-0.61], device=dev())
    for b, c, nb in ((major, 1, major), (major, 1, 1), (1, major, 1)):
        nz = synth.tensor(f'ufdk/{U.row_id(row)}/n{nb}', (nb, 1, oh, ow)).to(dev())
        out = torch.empty((b, c, oh, ow), dtype=torch.float32, device=dev())
        sel = _native.lib().fmgan_blur_noise_bias_act_select(p0, out.data_ptr(), nz.data_ptr(), b, c, in_h, in_w, ps, rs,
                                                             kh, kw, px0, px1, py0, py1)
        assert sel == kernel, f'{U.row_id(row)}: the fused select says {sel}'
        for bias in (synth.tensor(f'ufdk/{U.row_id(row)}/b', (c,)).to(dev()), None):
            ref = _native.noise_bias_act(y2.view(b, c, oh, ow), nz, nw, bias, 0.2, 2 ** 0.5)
            y = _fused_blur(p0, dev(), b, c, in_h, in_w, ps, rs, kd, row[7:], nz, nw, bias, 0.2, 2 ** 0.5)
            assert not torch.isnan(y).any()
            assert torch.equal(y, ref), f'b={b} c={c} noise batch {nb} bias {bias is not None}'


# --------------------------------------------------------------------------------------------- seeded sweeps, per kernel
def _draw(rng, kernel):
    """One draw from the kernel's own domain (f32, minor 1, down 1, 1..4 taps; pads independent in -2..6), sized inside the
    kernel's rules, or None where the input or the output would be empty (the caller redraws)."""
    kh, kw = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    px0, px1, py0, py1 = (int(v) for v in rng.integers(-2, 7, 4))
    major = int(rng.integers(1, 7))
    if kernel == 3:
        up = 2
        in_h, in_w = int(rng.integers(1, 41)), int(rng.integers(1, 81))
    else:
        up = 1
        if kernel == 1:                                   # out_w >= 64 and out_h >= 4
            oh, ow = int(rng.integers(4, 41)), int(rng.integers(64, 301))
        elif rng.integers(0, 2) == 0:                     # plane-tile: a wide plane of fewer than 4 output rows ...
            oh, ow = int(rng.integers(1, 4)), int(rng.integers(64, 301))
        else:                                             # ... or rows below 64 columns
            oh, ow = int(rng.integers(1, 41)), int(rng.integers(1, 64))
        in_h, in_w = oh - py0 - py1 + kh - 1, ow - px0 - px1 + kw - 1
        if in_h <= 0 or in_w <= 0:
            return None
        if kernel == 2 and in_h * in_w <= 256 and rng.integers(0, 2) == 0:
            major *= 700                                  # enough planes for several per block (pb > 1)
    return (kernel, major, in_h, in_w, kh, kw, up, px0, px1, py0, py1)


@pytest.mark.parametrize('kernel', [1, 2, 3])
def test_upfirdn2d_random_arguments_per_kernel(kernel):
    """25 seeded draws from each fast kernel's own domain, the four pads drawn independently: every accepted draw must select
    that kernel (a draw that selects another one fails; none is skipped) and match the oracle."""
    from op import _native
    rng = np.random.default_rng(7000 + kernel)
    done = 0
    while done < 25:
        row = _draw(rng, kernel)
        if row is None:
            continue
        _, major, in_h, in_w, kh, kw, up, px0, px1, py0, py1 = row
        oh, ow = _native.upfirdn2d_out_size(in_h, in_w, kh, kw, up, up, 1, 1, px0, px1, py0, py1)
        if oh <= 0 or ow <= 0 or in_h * up + py0 + py1 <= 0 or in_w * up + px0 + px1 <= 0:
            continue                                       # the Python-side out-size check (_native.upfirdn2d raises)
        sel = _select(row)
        assert sel == kernel, f'draw {done} {U.row_id(row)}: select says {sel}'
        x = rng.standard_normal((major, in_h, in_w)).astype(np.float32)
        k = rng.standard_normal((kh, kw)).astype(np.float32)
        ref = _oracle(torch.from_numpy(x), torch.from_numpy(k), row)
        y = _run(torch.from_numpy(x).to(dev()), torch.from_numpy(k).to(dev()), row)
        assert tuple(y.shape) == (major, oh, ow)
        np.testing.assert_allclose(y.cpu().numpy(), ref, err_msg=f'draw {done} {U.row_id(row)}', **_tol(np.abs(ref).max()))
        done += 1
