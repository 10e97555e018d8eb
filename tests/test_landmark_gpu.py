"""GPU tests of the landmark stages (csrc/landmark.hip through op/landmark.py and Util/landmark_util.py): the kernels
against the reference's recorded results (tests/golden/landmark.npz; cases and bounds in tests/landmark_cases.py, the
checks themselves in tests/landmark_checks.py, shared with the CPU run of the composites), sizes at which the kernels
take another path, and the launch counts the stages promise."""
import numpy as np
import pytest
import torch

import landmark_cases as lc
import landmark_checks as checks
import launches
import synth
from gpumem import dev, misaligned

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(lc.CROP_CASES))
def test_crop_kernels_match_reference(name, golden):
    from op import landmark as L
    c = lc.CROP_CASES[name]
    assert L.face_crop_serves(lc.crop_image(name).to(dev()), c['r'])
    with launches.observed() as rec:
        checks.crop(name, dev(), golden)
    # three forwards (two runs and the zero image's) and three backwards (two runs and the all-ones gradient's), one
    # launch each, nothing else
    n, _, h, w = c['shape']
    assert rec.names == ['face_crop'] * 6
    assert [i[4] for i in rec.infos('face_crop')] == [0, 1, 0, 1, 1, 0] and {i[:4] for i in rec.infos('face_crop')} == {(n, h, w, c['r'])}


# (ux, uy, bx, by) on a [4, 3, 37, 45] image, 32 x 32 crops: a 5 x 7 canvas (up by more than 4), a box wholly outside the
# image, the image exactly, the last row of the image inside a 90 x 70 canvas
EDGE_BOXES = [(10, 12, 17, 17), (60, -40, 90, -10), (0, 0, 45, 37), (-30, 36, 40, 126)]


def test_crop_kernels_edge_boxes_against_float64():
    """Boxes the fixture does not hold, against the closed form in float64.  Bound: crop_small's, as a fraction of the
    value range (the same arithmetic on the same value range forward; backward the range grows with the number of output
    pixels a source pixel feeds)."""
    from op import landmark as L
    c = lc.CROP_CASES['crop_small']
    img = synth.tensor('landmark/edge/img', (4, 3, 37, 45), dist='uniform')
    go = synth.tensor('landmark/edge/go', (4, 3, 32, 32))
    x = img.to(dev()).requires_grad_(True)
    out = L.face_crop(x, EDGE_BOXES, 32)
    grad, = torch.autograd.grad(out, x, go.to(dev()))
    x64 = img.double().requires_grad_(True)
    twin = L.face_crop_composite(x64, EDGE_BOXES, 32)
    twin_grad, = torch.autograd.grad(twin, x64, go.double())
    checks._within('edge boxes forward', out, twin, lc.bound(c['fwd_ref_err'], c['fwd_range']))
    rng = float(twin_grad.abs().max())
    checks._within('edge boxes backward', grad, twin_grad, lc.bound(c['bwd_ref_err'] * rng / c['bwd_range'], rng))
    assert not bool(out[1].any()) and not bool(grad[1].any())            # wholly outside: a zero crop, a zero gradient
    assert int((grad[3] != 0).sum()) > 0 and not bool(grad[3, :, :36].any())
    # an empty box reaches the kernel only in a device tensor (host boxes are refused): zeros, no fault
    empty = torch.tensor([(5, 5, 5, 9)] * 4, dtype=torch.int32, device=dev())
    assert not bool(L.face_crop(x.detach(), empty, 32).any())
    with pytest.raises(ValueError, match='side'):
        L.face_crop(x.detach(), [(5, 5, 5, 9)] * 4, 32)


def test_detector_input_kernel():
    from op import landmark as L
    for shape in ((2, 3, 64, 56), (1, 3, 7, 9)):                         # planes of a multiple of 4 elements, and not
        img = synth.tensor('landmark/det', shape, dist='uniform')
        with launches.observed() as rec:
            got = L.detector_input(misaligned(img.to(dev())))
        assert rec.names == ['detector_input']
        assert torch.equal(got.cpu(), L.detector_input_composite(img))


@pytest.mark.parametrize('name', sorted(lc.DECODE_CASES))
def test_decode_kernel_matches_reference(name, golden):
    with launches.observed() as rec:
        checks.decode(name, dev(), golden)
    assert rec.names == ['landmark_decode'] * 3


def test_decode_is_one_launch_whatever_the_map_count():
    from op import landmark as L
    for b, c in ((1, 1), (3, 7), (4, 68)):
        hm = synth.tensor(f'landmark/decode_n/{b}x{c}', (b, c, 64, 64))
        hm[0, 0, 63, 62:] = float('nan')                                   # NaN is the maximum, its first index wins
        center = synth.tensor('landmark/decode_n/center', (b, 2), dist='uniform', scale=60.0, shift=128.0)
        scale = synth.tensor('landmark/decode_n/scale', (b,), dist='uniform', scale=0.8, shift=1.6)
        with launches.observed() as rec:
            preds, orig = L.landmark_decode(misaligned(hm.to(dev())), center.to(dev()), scale.to(dev()))
        assert rec.names == ['landmark_decode'] and rec.infos('landmark_decode') == [(b, c)]
        want, want_orig = L.landmark_decode_composite(hm, center, scale)
        assert torch.equal(preds.cpu(), want) and preds[0, 0].tolist() == [62.5, 63.5]
        # the closed form on both sides; a value within float rounding of an integer may truncate either way
        off = (orig.cpu() - want_orig).abs()
        assert float(off.max()) <= 1 and int((off != 0).sum()) <= 1


def test_distance_kernels_match_reference(golden):
    with launches.observed() as rec:
        checks.distance(dev(), golden)
    # three forwards; backwards: both gradients in one launch, then the one of b alone
    assert rec.names.count('heatmap_distance') == len(rec.names) == 5
    assert [i[2] for i in rec.infos('heatmap_distance')] == [0, 1, 0, 0, 1]


@pytest.mark.parametrize('shape', [(2, 5, 36, 36), (3, 1, 10, 10), (1, 2, 64, 64)])
def test_distance_kernels_partial_blocks_and_alignment(shape):
    """Samples of 6480 (two partials, the second not full), 100 and 8192 elements, from pointers 4 bytes off a 16-byte
    boundary, against float64.  Bound: the reference's relative error at the fixture's case, times the margin."""
    from op import landmark as L
    c = lc.DISTANCE_CASE
    a, b = synth.tensor('landmark/dist2/a', shape), synth.tensor('landmark/dist2/b', shape)
    g = synth.tensor('landmark/dist2/g', shape[:1])
    x, y = misaligned(a.to(dev())).requires_grad_(True), misaligned(b.to(dev()))
    assert L.heatmap_distance_serves(x, y)
    d = L.heatmap_distance(x, y)
    gx, = torch.autograd.grad(d, x, g.to(dev()))
    want = torch.sum(torch.square(a.double() - b.double()), dim=(1, 2, 3))
    rng = float(want.max())
    checks._within('distance', d, want, lc.bound(c['out_ref_err'] * rng / c['out_range'], rng))
    want_g = 2 * g.double().view(-1, 1, 1, 1) * (a.double() - b.double())
    rng = float(want_g.abs().max())
    checks._within('its gradient', gx, want_g, lc.bound(c['grad_ref_err'] * rng / c['grad_range'], rng))
    # a sample of 4k + 2 elements goes to the composite
    odd = torch.zeros(2, 1, 3, 2, device=dev())
    assert not L.heatmap_distance_serves(odd, odd) and tuple(L.heatmap_distance(odd, odd + 1).tolist()) == (6.0, 6.0)


def test_heatmap_and_loss_match_reference(golden, monkeypatch):
    from Util.landmark_util import Get_HeatMap_PyTorch
    fa = checks.heatmap_and_loss(dev(), golden, monkeypatch)
    with launches.observed() as rec:
        Get_HeatMap_PyTorch(lc.e2e_images('g').to(dev()), fa, dev())
    assert rec.names == ['detector_input', 'face_crop']                  # one crop launch for the batch


def test_g_step_adds_the_term_only_past_the_threshold(monkeypatch):
    checks.g_step(dev(), monkeypatch)


def test_edit_scores_fill_the_heatmap_and_landmark_slots(monkeypatch):
    checks.edit_scores(dev(), monkeypatch)


def test_composite_switch_keeps_the_kernels_out(monkeypatch):
    from op import landmark as L
    monkeypatch.setattr(L, 'LANDMARK_FUSE', False)
    img = lc.crop_image('crop_small').to(dev())
    hm = lc.decode_maps('decode_border').to(dev())
    with launches.observed() as rec:
        out = L.face_crop(img, lc.CROP_CASES['crop_small']['box'], 32)
        L.detector_input(img)
        L.heatmap_distance(hm, hm)
        L.landmark_decode(hm)
    assert rec.names == []
    fused = L.face_crop(img, lc.CROP_CASES['crop_small']['box'], 32, fuse=True)
    c = lc.CROP_CASES['crop_small']
    np.testing.assert_allclose(out.cpu().numpy(), fused.cpu().numpy(), rtol=0, atol=2 * lc.bound(c['fwd_ref_err'], c['fwd_range']))
