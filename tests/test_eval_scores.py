"""GPU tests of the evaluation's metric-stage kernel (csrc/eval_scores.hip, op/eval_scores.py): grey images bit for bit
against a numpy fp32 emulation of the stated order (and against the reference's own conversion, tests/golden/face_id.npz),
the L1 partial sums against float64, guarded output buffers, and what the binding refuses."""
import numpy as np
import pytest
import torch

import synth
from gpumem import dev, guarded, guards_intact, misaligned

pytestmark = pytest.mark.gpu


def emulate_gray(x, k):
    """numpy fp32, the order csrc/eval_scores.hip states: g = (c0*x0 + c1*x1) + c2*x2 with separately rounded products;
    window sum serial from 0, rows top to bottom, columns left to right; times 1/k^2."""
    x = np.asarray(x, dtype=np.float32)
    c = np.array([0.2989, 0.587, 0.114], dtype=np.float32)
    g = (c[0] * x[:, 0] + c[1] * x[:, 1]) + c[2] * x[:, 2]
    assert g.dtype == np.float32
    acc = np.zeros((x.shape[0], x.shape[2] // k, x.shape[3] // k), dtype=np.float32)
    for r in range(k):
        for col in range(k):
            acc = acc + g[:, r::k, col::k]
    return (acc * np.float32(1.0 / (k * k)))[:, None]


def launch(a, b, k, want_gray_a=True, want_gray_b=False, want_l1=False):
    """fmgan_face_input_f32 into guarded buffers pre-filled with NaN: (gray_a, gray_b, l1 per sample), after checking
    that no guard word changed and every requested element was written."""
    from op import _native
    L = _native.lib()
    n, _, h, w = a.shape
    blocks = L.fmgan_face_input_blocks(n, h, w, k)
    assert blocks > 0
    bufs = {}
    if want_gray_a:
        bufs['ga'] = guarded((n, 1, h // k, w // k))
    if want_gray_b:
        bufs['gb'] = guarded((n, 1, h // k, w // k))
    if want_l1:
        bufs['l1'] = guarded((n, blocks))
    p = {key: v[1].data_ptr() for key, v in bufs.items()}
    st = L.fmgan_face_input_f32(_native.fp(a), _native.fp(b), p.get('ga'), p.get('gb'), p.get('l1'), n, h, w, k,
                                torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    for key, (buf, view) in bufs.items():
        assert guards_intact(buf), key
    out = {key: v[1] for key, v in bufs.items()}
    l1 = out['l1'].sum(1) / (3 * h * w) if want_l1 else None
    return out.get('ga'), out.get('gb'), l1


def _pair(tag, shape):
    a = synth.tensor(f'eval_scores/{tag}/a', shape, dist='uniform').to(dev())
    b = synth.tensor(f'eval_scores/{tag}/b', shape, dist='uniform').to(dev())
    return a, b


SHAPES = [((2, 3, 128, 128), 1, False), ((2, 3, 256, 256), 2, False), ((1, 3, 512, 512), 4, False),
          ((1, 3, 1024, 1024), 8, False), ((3, 3, 6, 10), 2, False), ((1, 3, 8, 24), 8, False),
          ((2, 3, 64, 64), 2, True),
          # W % 4 != 0 at k = 1 (a unit's last columns lie past the row's end) and more than one block at k = 4
          ((2, 3, 5, 7), 1, False), ((2, 3, 40, 132), 4, False),
          # many samples: grid.x = batch * blocks, far more blocks than one wave of them on the chip
          ((70000, 3, 2, 4), 2, False)]


@pytest.mark.parametrize('shape,k,misalign', SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gray_and_l1_against_emulation(shape, k, misalign):
    """Both grey images equal the numpy emulation exactly; L1 is within rtol 1e-5 of float64 (the kernel's longest chain is
    40 additions of non-negative terms: 2.4e-6, the host sum of the few partials adds less than that again); the one-image
    launch gives the same grey image; no guard word is touched and no output element is left unwritten."""
    a, b = _pair('x'.join(map(str, shape)) + f'/{k}', shape)
    if misalign:
        a, b = misaligned(a), misaligned(b)
    ga, gb, l1 = launch(a, b, k, want_gray_b=True, want_l1=True)
    assert not torch.isnan(ga).any() and not torch.isnan(gb).any() and not torch.isnan(l1).any()
    np.testing.assert_array_equal(ga.cpu().numpy(), emulate_gray(a.cpu().numpy(), k))
    np.testing.assert_array_equal(gb.cpu().numpy(), emulate_gray(b.cpu().numpy(), k))
    want = (a.double() - b.double()).abs().mean((1, 2, 3))
    np.testing.assert_allclose(l1.double().cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=0)
    alone, none_b, none_l1 = launch(a, None, k)
    assert torch.equal(alone, ga) and none_b is None and none_l1 is None
    only_l1 = launch(a, b, k, want_gray_a=False, want_l1=True)
    assert only_l1[0] is None and torch.equal(only_l1[2], l1)


def test_gray_equals_the_reference_conversion(golden):
    """At [2,3,256,256] the kernel's grey images are the reference's Convert_Tensor_For_Face_Recognition_Loss output
    (tests/golden/face_id.npz['converted']) bit for bit, through the binding and through op.eval_scores.face_input."""
    import cases
    from op import _native, eval_scores as ES
    c = cases.FACE_ID_CASE
    a = synth.tensor(c['name'] + '/a', (c['b'], 3, c['size'], c['size']), dist='uniform').to(dev())
    b = synth.tensor(c['name'] + '/b', (c['b'], 3, c['size'], c['size']), dist='uniform').to(dev())
    assert ES.face_input_serves(a, b)
    ga, gb, l1 = _native.face_input(a, b, want_gray_b=True, want_l1=True)
    np.testing.assert_array_equal(ga.cpu().numpy(), golden('face_id')['converted'])
    comp = ES.face_input_composite(a, b, want_gray_b=True, want_l1=True)
    assert torch.equal(gb, comp[1]) and torch.equal(ga, comp[0])
    torch.testing.assert_close(l1, comp[2], rtol=1e-5, atol=0)
    fused = ES.face_input(a, b, want_gray_b=True, want_l1=True)
    assert torch.equal(fused[0], ga) and torch.equal(fused[1], gb) and torch.equal(fused[2], l1)
    assert _native.face_input(a)[1:] == (None, None)


@pytest.mark.parametrize('size,k', [(128, 1), (256, 2), (512, 4), (1024, 8)])
def test_binding_pools_to_the_face_size(size, k):
    """The binding derives k = W // 128 as Convert_Tensor_For_Face_Recognition_Loss does: 128^2 grey images at every size,
    equal to the composite on the same device bit for bit."""
    from op import _native, eval_scores as ES
    a, b = _pair(f'bind/{size}', (1, 3, size, size))
    ga, gb, l1 = _native.face_input(a, b, want_gray_b=True, want_l1=True)
    assert tuple(ga.shape) == tuple(gb.shape) == (1, 1, 128, 128) and tuple(l1.shape) == (1,)
    np.testing.assert_array_equal(ga.cpu().numpy(), emulate_gray(a.cpu().numpy(), k))
    comp = ES.face_input_composite(a, b, want_gray_b=True, want_l1=True)
    assert torch.equal(ga, comp[0]) and torch.equal(gb, comp[1])
    torch.testing.assert_close(l1, comp[2], rtol=1e-5, atol=0)


def test_l1_is_exact_zero_reproducible_and_the_same_in_both_load_forms():
    a, b = _pair('l1', (2, 3, 64, 64))
    _, _, zero = launch(a, a, 2, want_gray_a=False, want_l1=True)
    assert torch.equal(zero, torch.zeros_like(zero))
    first = launch(a, b, 2, want_gray_b=True, want_l1=True)
    again = launch(a, b, 2, want_gray_b=True, want_l1=True)
    scalar = launch(misaligned(a), misaligned(b), 2, want_gray_b=True, want_l1=True)
    mixed = launch(misaligned(a), b, 2, want_gray_b=True, want_l1=True)          # one misaligned pointer is enough
    for other in (again, scalar, mixed):
        for x, y in zip(first, other):
            assert torch.equal(x, y)


def test_nan_in_b_stays_out_of_gray_a():
    a, b = _pair('nan', (2, 3, 64, 64))
    b[1, 2, 10, 20] = float('nan')
    ga, gb, l1 = launch(a, b, 2, want_gray_b=True, want_l1=True)
    np.testing.assert_array_equal(ga.cpu().numpy(), emulate_gray(a.cpu().numpy(), 2))
    nan = torch.isnan(gb)
    assert int(nan.sum()) == 1 and bool(nan[1, 0, 5, 10])
    assert not torch.isnan(l1[0]) and torch.isnan(l1[1])


def test_binding_refuses_what_the_kernel_cannot_read():
    from op import _native, eval_scores as ES
    a, b = _pair('refuse', (2, 3, 64, 64))
    for bad in (a.double(), a.bfloat16(), a.cpu()):
        with pytest.raises(RuntimeError):
            _native.face_input(bad)
        with pytest.raises((RuntimeError, ValueError)):
            _native.face_input(a, bad, want_l1=True)
        assert not ES.face_input_serves(bad) and not ES.face_input_serves(a, bad)
    strided = _pair('refuse/wide', (2, 3, 64, 128))[0][..., ::2]
    assert tuple(strided.shape) == (2, 3, 64, 64) and not strided.is_contiguous()
    with pytest.raises(RuntimeError, match='contiguous'):
        _native.face_input(strided)
    with pytest.raises(RuntimeError, match='contiguous'):
        _native.face_input(a, strided, want_gray_b=True)
    four = torch.zeros(2, 4, 64, 64, device=dev())
    with pytest.raises(ValueError):
        _native.face_input(four)
    with pytest.raises(ValueError):
        _native.face_input(a, b[:1], want_l1=True)
    with pytest.raises(ValueError):
        _native.face_input(a, want_gray_b=True)
    # the op routes such tensors to the composite instead
    got = ES.face_input(strided, b, want_gray_b=True, want_l1=True)
    want = ES.face_input_composite(strided, b, want_gray_b=True, want_l1=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    with pytest.raises(RuntimeError, match='inference only'):
        ES.face_input(a.clone().requires_grad_(True), b)


def test_unsupported_pooling_factor_takes_the_composite():
    """A 390^2 image pools by 3: the library refuses (fmgan_face_input_blocks = 0, the binding returns None) and
    face_input gives the composite's tensors."""
    from op import _native, eval_scores as ES
    a, b = _pair('k3', (1, 3, 390, 390))
    assert _native.face_input_pool(390) == 3 and _native.lib().fmgan_face_input_blocks(1, 390, 390, 3) == 0
    assert _native.face_input(a, b, want_gray_b=True, want_l1=True) is None
    assert not ES.face_input_serves(a, b)
    got = ES.face_input(a, b, want_gray_b=True, want_l1=True)
    want = ES.face_input_composite(a, b, want_gray_b=True, want_l1=True)
    assert tuple(got[0].shape) == (1, 1, 130, 130)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
