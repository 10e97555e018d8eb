"""The checks of the landmark stages, written once for both devices (not a conftest: plain helpers, imported by name):
tests/test_landmark.py runs them on the CPU, where every stage is its composite, tests/test_landmark_gpu.py on the GPU,
where every stage is its kernel.  Every figure is printed before it is asserted."""
import sys

import numpy as np
import torch
from torch import nn

import landmark_cases as lc


def _max_err(got, want):
    return float((got.detach().double().cpu() - torch.as_tensor(want).detach().double()).abs().max())


def _within(what, got, want, limit):
    e = _max_err(got, want)
    print(f'{what}: max |error| {e:.3e}, bound {limit:.3e}')
    assert e <= limit, f'{what}: {e:.3e} above {limit:.3e}'


def patch_package(monkeypatch):
    """The stand-in `face_alignment` modules (get_predictions) into sys.modules for one test."""
    for name, mod in lc.stub_modules().items():
        monkeypatch.setitem(sys.modules, name, mod)


# ----------------------------------------------------------------------------- crop
def crop(name, device, golden):
    from op import landmark as L
    from Util.landmark_util import Face_Crop_Boxes
    c = lc.CROP_CASES[name]
    r, st = c['r'], c['stride']
    fx = golden('landmark')
    box = Face_Crop_Boxes(*lc.crop_center_scale(name), r)
    assert box.dtype == torch.int32 and [tuple(b) for b in box.tolist()] == [tuple(b) for b in c['box']]
    fwd, bwd = lc.bound(c['fwd_ref_err'], c['fwd_range']), lc.bound(c['bwd_ref_err'], c['bwd_range'])
    img = lc.crop_image(name).to(device).requires_grad_(True)
    go = lc.crop_grad(name).to(device)
    out = L.face_crop(img, box, r)
    grad, = torch.autograd.grad(out, img, go)
    assert tuple(out.shape) == (c['shape'][0], 3, r, r) and tuple(grad.shape) == tuple(c['shape'])
    _within(f'{name} forward against the fixture', out[:, :, ::st, ::st], fx[f'{name}/out'], fwd)
    _within(f'{name} backward against the fixture', grad[:, :, ::st, ::st], fx[f'{name}/grad'], bwd)
    # the whole tensors against the closed form in float64 (what the fixture tool measured the reference against)
    img64 = lc.crop_image(name).double().requires_grad_(True)
    twin = L.face_crop_composite(img64, box, r)
    twin_grad, = torch.autograd.grad(twin, img64, lc.crop_grad(name).double())
    _within(f'{name} forward against the float64 closed form', out, twin, fwd)
    _within(f'{name} backward against the float64 closed form', grad, twin_grad, bwd)
    # exactly 0 outside the crops
    outside = torch.ones(c['shape'], dtype=torch.bool)
    for i, (ux, uy, bx, by) in enumerate(c['box']):
        outside[i, :, max(uy, 0):max(by, 0), max(ux, 0):max(bx, 0)] = False
    assert bool((grad.cpu()[outside] == 0).all())
    assert name != 'crop_small' or int(outside.sum()) > 0
    # two runs, the same bits
    out2 = L.face_crop(img, box, r)
    grad2, = torch.autograd.grad(out2, img, go, retain_graph=True)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    # the crop is affine in the image: sum(crop(x)) - sum(crop(0)) = <backward of all ones, x>
    ones, = torch.autograd.grad(out2, img, torch.ones_like(out2))
    zero = L.face_crop(torch.zeros_like(img), box, r)
    lhs = float(out.detach().double().sum() - zero.double().sum())
    rhs = float((ones.double() * img.detach().double()).sum())
    limit = 2 * out.numel() * fwd + img.numel() * lc.bound(c['bwd_ref_err'], float(ones.abs().max()))
    print(f'{name} adjoint: {lhs:.9e} against {rhs:.9e}, bound {limit:.3e}')
    assert abs(lhs - rhs) <= limit
    return out, grad


# ----------------------------------------------------------------------------- decode
def decode(name, device, golden):
    from Util.landmark_util import Get_Preds_FromHeatMap_PyTorch
    fx = golden('landmark')
    hm = lc.decode_maps(name).to(device)
    center, scale = lc.decode_center_scale(name)
    preds, preds_orig = Get_Preds_FromHeatMap_PyTorch(hm, device, [center[0], center[1]], [float(scale[0]), float(scale[1])])
    assert tuple(preds.shape) == tuple(preds_orig.shape) == (2, 5, 2) and preds.device == hm.device
    np.testing.assert_array_equal(preds.cpu().numpy(), fx[f'{name}/preds'])
    np.testing.assert_array_equal(preds_orig.cpu().numpy(), fx[f'{name}/preds_orig'])
    for m, want in enumerate(lc.decode_expected_preds(name)):
        assert want is None or tuple(preds[m // 5, m % 5].tolist()) == want, (m, want)
    # tensors in place of the lists give the same; without center and scale preds_orig is zeros
    p2, o2 = Get_Preds_FromHeatMap_PyTorch(hm, device, center.to(device), scale.to(device))
    assert torch.equal(p2, preds) and torch.equal(o2, preds_orig)
    p3, o3 = Get_Preds_FromHeatMap_PyTorch(hm, device)
    assert torch.equal(p3, preds) and not bool(o3.any())


# ----------------------------------------------------------------------------- distance
def distance(device, golden):
    from op import landmark as L
    c = lc.DISTANCE_CASE
    fx = golden('landmark')
    st = c['stride']
    a, b, g = (t.to(device) for t in lc.distance_inputs())
    a.requires_grad_(True)
    b.requires_grad_(True)
    d = L.heatmap_distance(a, b)
    ga, gb = torch.autograd.grad(d, (a, b), g)
    _within('distance forward against the fixture', d, fx['dist/out'], lc.bound(c['out_ref_err'], c['out_range']))
    gbound = lc.bound(c['grad_ref_err'], c['grad_range'])
    _within('distance grad_a against the fixture', ga[:, :, ::st, ::st], fx['dist/grad_a'], gbound)
    _within('distance grad_b against the fixture', gb[:, :, ::st, ::st], -fx['dist/grad_a'], gbound)
    a64, b64, g64 = (t.double() for t in lc.distance_inputs())
    want = 2 * g64.view(-1, 1, 1, 1) * (a64 - b64)
    _within('distance grad_a against float64', ga, want, gbound)
    _within('distance grad_b against float64', gb, -want, gbound)
    assert torch.equal(gb, -ga)
    d2 = L.heatmap_distance(a, b)
    assert torch.equal(d, d2)
    # a heat map without a gradient gets none
    a0 = a.detach()
    d3 = L.heatmap_distance(a0, b)
    assert torch.equal(d3, d)
    d3.backward(g)
    assert a0.grad is None and torch.equal(b.grad, gb)


# ----------------------------------------------------------------------------- end to end
def heatmap_and_loss(device, golden, monkeypatch):
    from Util.landmark_util import Get_HeatMap_PyTorch
    from Util.training_util import Heat_Map_Loss
    patch_package(monkeypatch)
    c = lc.E2E
    fx = golden('landmark')
    fa = lc.Alignment(device)
    g_output = lc.e2e_images('g').to(device).requires_grad_(True)
    r_input = lc.e2e_images('r').to(device)
    heatmap, center_list, scale_list = Get_HeatMap_PyTorch(g_output, fa, device)
    assert tuple(heatmap.shape) == (c['shape'][0], c['maps'], 64, 64) and heatmap.requires_grad
    np.testing.assert_array_equal(np.stack([x.numpy() for x in center_list]), fx['e2e/center'])
    np.testing.assert_array_equal(np.asarray(scale_list, dtype=np.float64), fx['e2e/scale'])
    st = c['hm_stride']
    _within('heat maps against the fixture', heatmap[:, :, ::st, ::st], fx['e2e/heatmap'],
            lc.bound(c['hm_ref_err'], c['hm_range']))
    loss = Heat_Map_Loss(g_output, r_input, fa, device)
    grad, = torch.autograd.grad(loss, g_output)
    _within('Heat_Map_Loss against the fixture', loss, fx['e2e/loss'], lc.bound(c['loss_ref_err'], c['loss_range']))
    _within('its gradient against the fixture', grad, fx['e2e/grad'], lc.bound(c['grad_ref_err'], c['grad_range']))
    return fa


class _Forward:
    """Stand-in for Forward_Inference_3_Encoder: image = G(photo) + 0.25 * render, G a 1 x 1 convolution."""

    def __call__(self, p, r, e_tsr, e_w, e_wp, g, *args, **kwargs):
        return getattr(g, 'module', g)(p) + 0.25 * r


def g_step(device, monkeypatch):
    """G_Loss_BackProp adds the heat-map term only with an fa_model and past the threshold."""
    import train_3_encoder as T
    from Util.training_util import Heat_Map_Loss
    patch_package(monkeypatch)
    monkeypatch.setattr(T, 'Forward_Inference_3_Encoder', _Forward())
    fa = lc.Alignment(device)
    torch.manual_seed(0)
    G = nn.Conv2d(3, 3, 1).to(device)
    enc = [nn.Linear(2, 2).to(device) for _ in range(3)]
    D = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(3, 1)).to(device)
    photo, render = lc.e2e_images('g').to(device), lc.e2e_images('r').to(device)
    assert T.default_args().hmap_loss_lambda == 0 and T.default_args().hmap_iter_thres == np.inf

    def run(fa_model, iter_idx, **over):
        args = T.default_args(**{'hmap_loss_lambda': 0.5, 'hmap_iter_thres': 10, **over})
        ld = {}
        T.G_Loss_BackProp(G, *enc, D, photo, render, photo, args, ld, None, None, None, fa_model, iter_idx)
        return ld, G.weight.grad.clone()

    def same(a, b):          # the convolution's weight gradient is not bit-reproducible on every device
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5 * float(b.abs().max()))
        return True
    base, grad_base = run(None, 11)
    assert float(base['hmap']) == 0 and base['hmap'].ndim == 0
    at, grad_at = run(fa, 10)                                  # not past the threshold: iter_idx > thres is the rule
    assert float(at['hmap']) == 0 and same(grad_at, grad_base)
    default, grad_default = run(fa, 10 ** 9, hmap_iter_thres=np.inf)
    assert float(default['hmap']) == 0 and same(grad_default, grad_base)
    past, grad_past = run(fa, 11)
    with torch.no_grad():
        want = 0.5 * Heat_Map_Loss(_Forward()(photo, render, None, None, None, G), render, fa, device)
    assert float(past['hmap'].detach()) > 0
    # the same operations with and without a graph: equal up to the convolutions' choice of algorithm
    torch.testing.assert_close(past['hmap'].detach(), want, rtol=1e-5, atol=0)
    moved = float((grad_past - grad_base).abs().max() / grad_base.abs().max())
    print(f'g step: the heat-map term moves the weight gradient by {moved:.3e} of its size')
    assert moved > 1e-3                                        # a hundred times what `same` allows


def _code(p):
    return 0.5 * p.mean((2, 3), keepdim=True)


class _TinyFace(nn.Module):
    def forward(self, x):
        return nn.functional.adaptive_avg_pool2d(x, (2, 3)).reshape(x.shape[0], 6) + 0.1


def edit_scores(device, monkeypatch):
    """Get_Edit_Score fills slots 3 and 4 with an fa_model, leaves them None without, and refuses an object()."""
    import pytest
    from Evaluation import quant_eval as QE
    from Util.landmark_util import Get_HeatMap_Landmark_PyTorch
    patch_package(monkeypatch)
    monkeypatch.setattr(QE, 'Encode_Photo', lambda p, e_tsr, e_wp, tsr_encode='Photo Image': _code(p))
    monkeypatch.setattr(QE, 'Forward_Inference_Reanimate', lambda code, r, *a, **k: code + 0.25 * r)
    monkeypatch.setattr(QE, 'Forward_Inference_3_Encoder', lambda p, r, *a, **k: _code(p) + 0.25 * r)
    monkeypatch.setattr(QE, 'face_region_scores',
                        lambda r, g: torch.mean(torch.square((r - g) * (r.mean(1, keepdim=True) > -1)), dim=(1, 2, 3)))
    fa = lc.Alignment(device)
    photo, r1, r2 = lc.e2e_images('g'), lc.e2e_images('r'), lc.e2e_images('r').flip(-1)
    loader = [[photo, r1, r2], [photo[:2], r2[:2]]]
    models = (None,) * 4
    none = QE.Get_Edit_Score(loader, device, models, (_TinyFace(), None, None))
    assert none[2] is None and none[3] is None
    s = QE.Edit_Scores(loader, device, models, (_TinyFace(), None, fa))
    assert tuple(s['hmap'].shape) == tuple(s['lmark'].shape) == tuple(s['cos'].shape) == (8,)
    assert s['hmap'].device.type == torch.device(device).type
    got = QE.Get_Edit_Score(loader, device, models, (_TinyFace(), None, fa))
    assert got[0] == none[0] and got[1] is None and got[4] == none[4]
    assert got[2] == float(s['hmap'].double().mean()) and got[3] == float(s['lmark'].double().mean())
    assert got[2] > 0 and np.isfinite(got[3])
    # the first entries are render 1 of batch 1: restated from the pieces
    with torch.no_grad():
        p, r = photo.to(device), r1.to(device)
        hm_g, lm_g = Get_HeatMap_Landmark_PyTorch(_code(p) + 0.25 * r, fa, device)
        hm_r, lm_r = Get_HeatMap_Landmark_PyTorch(r, fa, device)
    assert tuple(lm_g.shape) == (3, lc.E2E['maps'], 2)
    # two float32 sums of 12288 non-negative terms in different orders: far inside the worst case n * 2^-24 = 7e-4
    torch.testing.assert_close(s['hmap'][:3], torch.sum(torch.square(hm_r - hm_g), dim=(1, 2, 3)), rtol=1e-5, atol=0)
    assert torch.equal(s['lmark'][:3], torch.mean(torch.square(lm_r - lm_g), dim=(1, 2)))
    with pytest.raises(ValueError, match='face_alignment'):
        QE.Get_Edit_Score(loader, device, models, (_TinyFace(), None, object()))
