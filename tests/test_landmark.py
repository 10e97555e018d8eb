"""CPU tests of the landmark stages (op/landmark.py, Util/landmark_util.py, csrc/landmark.hip): every stage's composite
against the reference's recorded results (tests/golden/landmark.npz, tools/make_golden_landmark.py; cases and bounds in
tests/landmark_cases.py), the callers on stand-in networks, and the host logic of the library's entry points."""
import ctypes
import sys

import pytest
import torch

import landmark_cases as lc
import landmark_checks as checks
from nets import lib

CPU = torch.device('cpu')


@pytest.mark.parametrize('name', sorted(lc.CROP_CASES))
def test_crop_composite_matches_reference(name, golden):
    checks.crop(name, CPU, golden)


@pytest.mark.parametrize('name', sorted(lc.DECODE_CASES))
def test_decode_composite_matches_reference(name, golden):
    checks.decode(name, CPU, golden)


def test_distance_composite_matches_reference(golden):
    checks.distance(CPU, golden)


def test_heatmap_and_loss_match_reference(golden, monkeypatch):
    checks.heatmap_and_loss(CPU, golden, monkeypatch)


def test_g_step_adds_the_term_only_past_the_threshold(monkeypatch):
    checks.g_step(CPU, monkeypatch)


def test_edit_scores_fill_the_heatmap_and_landmark_slots(monkeypatch):
    checks.edit_scores(CPU, monkeypatch)


def test_trainer_hands_the_alignment_model_to_the_g_step_and_to_evaluate(monkeypatch):
    import train_3_encoder as T
    from Evaluation import quant_eval as QE
    seen = {}
    monkeypatch.setattr(T, 'D_Loss_BackProp', lambda *a, **k: None)
    monkeypatch.setattr(T, 'D_Reg_BackProp', lambda *a, **k: torch.zeros(()))
    monkeypatch.setattr(T, 'G_Reg_BackProp', lambda *a, **k: (torch.zeros(()), None, 0))
    monkeypatch.setattr(T, 'accumulate', lambda *a, **k: None)
    monkeypatch.setattr(T, 'G_Loss_BackProp', lambda *a, **k: seen.update(g=a[13], iter_idx=a[14]))
    monkeypatch.setattr(QE, 'Get_Edit_Score', lambda loader, device, gen, models, **k: seen.update(e=models) or (1, 2, 3, 4, 5))
    fa, face = object(), torch.nn.Identity()
    for given in (None, fa):
        nets = {k: torch.nn.Linear(2, 2) for k in ('G', 'E_Tsr', 'E_W', 'E_W_Plus', 'D')}
        tr = T.Trainer(nets, T.default_args(), face_rec_model=face, fa_model=given)
        tr.step(None, None, None)
        scores = tr.evaluate(edit_eval_loader=[])
        assert seen['g'] is given and seen['iter_idx'] == 0 and seen['e'] == (face, None, given)
        assert (scores['hmap_score'], scores['lmark_score']) == (3, 4)


def test_transform_and_box_arithmetic():
    """transform() forward and inverse at the fallback box (values by hand from the formula), Crop_An_Image's centre and
    scale, and the single-image crop against the batch composite."""
    from op import landmark as L
    from Util import landmark_util as LU
    center, scale = LU.Box_Center_Scale(lc.FALLBACK_BBOX, lc.REFERENCE_SCALE)
    assert center.dtype == torch.float32 and center.tolist() == pytest.approx([127.5, 127.5 - 255 * 0.12], abs=1e-5)
    assert scale == 510 / 195
    # h = 200 * 510 / 195 = 523.08; forward: r/h * x + r * (-c/h + 1/2), inverse: (x - r * (-c/h + 1/2)) * h/r
    assert LU.transform([150.0, 60.0], center, scale, 256).tolist() == [139, 109]          # 139.01, 109.94
    assert LU.transform([1, 1], center, scale, 256, True).tolist() == [-131, -162]          # -131.99, -162.59
    assert LU.transform([256, 256], center, scale, 256, True).tolist() == [389, 358]
    img = lc.crop_image('crop_small')
    scaled = (img + 1) * 255 / 2
    bbox = [9.0, 12.0, 29.0, 37.0, 1.0]
    crop, c1, s1 = LU.Crop_An_Image(scaled[:1], bbox, 30.0, resolution=32)
    box = LU.Face_Crop_Boxes([c1], [s1], 32)
    assert tuple(crop.shape) == (1, 3, 32, 32) and torch.equal(crop / 255.0, L.face_crop(img[:1], box, 32))
    with pytest.raises(ValueError, match='empty'):
        L.face_crop(img[:1], [(5, 5, 5, 9)], 32)


def test_detection_needs_the_package_and_applies_the_fallback(monkeypatch):
    from op import landmark as L
    from Util import landmark_util as LU
    img = lc.e2e_images('g')
    fa = lc.Alignment()
    with monkeypatch.context() as m:
        m.setitem(sys.modules, 'face_alignment', None)            # absent, whatever is installed
        with pytest.raises(ImportError, match='face_alignment'):
            LU.Batch_Img_Face_Detection(img, fa.face_detector, CPU, scaled=False)
    checks.patch_package(monkeypatch)
    boxes = LU.Batch_Img_Face_Detection(img, fa.face_detector, CPU, scaled=False)
    assert [[float(v) for v in b[:4]] for b in boxes] == [[float(v) for v in b[:4]] for b in lc.E2E['bbox']]
    assert boxes[1] == lc.FALLBACK_BBOX and boxes[2] == lc.FALLBACK_BBOX
    again = LU.Batch_Img_Face_Detection((img + 1) * 255 / 2, fa.face_detector, CPU)         # the reference's [0, 255] form
    assert [list(map(float, b)) for b in again] == [list(map(float, b)) for b in boxes]
    want = ((img + 1) * 255 / 2).flip(1) - torch.tensor([104.0, 117.0, 123.0]).view(1, 3, 1, 1)
    assert torch.equal(L.detector_input(img), want)
    assert not L.detector_input(img.clone().requires_grad_(True)).requires_grad


def test_composites_are_the_path_off_the_kernels(monkeypatch):
    """No stage serves a CPU, float64 or non-contiguous tensor, and the module switch is read from the environment."""
    import importlib
    from op import landmark as L
    x = lc.crop_image('crop_small')
    hm = lc.decode_maps('decode_border')
    assert not L.face_crop_serves(x, 32) and not L.detector_input_serves(x)
    assert not L.heatmap_distance_serves(hm, hm) and not L.landmark_decode_serves(hm)
    assert L.LANDMARK_FUSE is True
    monkeypatch.setenv('FMGAN_NO_LANDMARK_FUSE', '1')
    try:
        assert importlib.reload(L).LANDMARK_FUSE is False
    finally:
        monkeypatch.delenv('FMGAN_NO_LANDMARK_FUSE')
        importlib.reload(L)
    # the decode composite takes other map sizes (the kernel does not): a maximum planted in a 16 x 12 map
    small = torch.zeros(1, 1, 16, 12)
    small[0, 0, 5, 7], small[0, 0, 5, 8], small[0, 0, 4, 7] = 2.0, 1.0, 1.0
    preds, orig = L.landmark_decode(small)
    assert preds.tolist() == [[[7 + 1 + 0.25 - 0.5, 5 + 1 - 0.25 - 0.5]]] and not bool(orig.any())


def test_entry_points_host_logic():
    """Plans and argument checks of the library's entry points, all before any HIP call (the pointers are placeholders)."""
    L = lib()
    fake = ctypes.c_void_p(0x1000)
    EINVAL, EUNSUP, EOVER = -1, -2, -4
    assert L.fmgan_face_crop_select(8, 256, 256, 256) == 1 and L.fmgan_face_crop_select(3, 48, 40, 32) == 1
    assert L.fmgan_face_crop_select(0, 256, 256, 256) == EINVAL and L.fmgan_face_crop_select(1, 256, 0, 256) == EINVAL
    assert L.fmgan_face_crop_select(1, 40000, 256, 256) == EOVER and L.fmgan_face_crop_select(1, 256, 256, 40000) == EOVER
    assert L.fmgan_face_crop_fwd_f32(None, fake, fake, 1, 8, 8, 8, None) == EINVAL
    assert L.fmgan_face_crop_fwd_f32(fake, None, fake, 1, 8, 8, 8, None) == EINVAL
    assert L.fmgan_face_crop_bwd_f32(fake, fake, None, 1, 8, 8, 8, None) == EINVAL
    assert L.fmgan_face_crop_bwd_f32(fake, fake, fake, 1, 8, 8, 1 << 20, None) == EOVER
    assert L.fmgan_detector_input_f32(None, fake, 1, 64, None) == EINVAL
    assert L.fmgan_detector_input_f32(fake, fake, 0, 64, None) == EINVAL
    assert L.fmgan_heatmap_distance_blocks(3, 4 * 4096) == 4 and L.fmgan_heatmap_distance_blocks(3, 4100) == 2
    assert L.fmgan_heatmap_distance_blocks(3, 4098) == 0 and L.fmgan_heatmap_distance_blocks(0, 4096) == 0
    assert L.fmgan_heatmap_distance_fwd_f32(fake, fake, fake, 3, 4098, None) == EUNSUP
    assert L.fmgan_heatmap_distance_fwd_f32(fake, None, fake, 3, 4096, None) == EINVAL
    assert L.fmgan_heatmap_distance_bwd_f32(fake, fake, fake, None, None, 3, 4096, None) == EINVAL
    assert L.fmgan_heatmap_distance_bwd_f32(fake, fake, fake, fake, None, 3, 1 << 50, None) == EOVER
    assert L.fmgan_landmark_decode_f32(fake, None, None, fake, fake, 2, 5, 32, 32, None) == EUNSUP
    assert L.fmgan_landmark_decode_f32(fake, fake, None, fake, fake, 2, 5, 64, 64, None) == EINVAL
    assert L.fmgan_landmark_decode_f32(fake, None, None, fake, None, 2, 5, 64, 64, None) == EINVAL
    assert L.fmgan_landmark_decode_f32(fake, None, None, fake, fake, 0, 5, 64, 64, None) == EINVAL
