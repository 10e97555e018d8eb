#!/usr/bin/env python3
"""Generate tests/golden/landmark.npz: the reference's Util/landmark_util.py and Heat_Map_Loss on CPU.

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_landmark.py
The reference's Util/landmark_util.py imports the third-party `face_alignment` package from a hard-coded path; stub modules
stand in for it (tests/landmark_cases.py: stub_modules), carrying this tool's own `transform` (the package's formula,
written out below in float32) and the stand-in `get_predictions`.  Nothing else of the reference is stubbed.

Recorded (outputs only; inputs and weights come from tests/synth.py and tests/landmark_cases.py on both sides):
  crop cases     Crop_PyTorch per sample behind Get_HeatMap_PyTorch's scaling and / 255 (`/out`), and autograd's gradient
                 with respect to the image for a seeded upstream gradient (`/grad`); every `stride`-th row and column
  decode cases   Get_Preds_FromHeatMap_PyTorch: `/preds`, `/preds_orig`
  distance       the sum of squares of Heat_Map_Loss (`dist/out`) and the gradient of its mean-free form for a seeded
                 upstream gradient (`dist/grad_a`, strided)
  end to end     Get_HeatMap_PyTorch (`e2e/heatmap`, strided), Heat_Map_Loss (`e2e/loss`) and its gradient with respect to
                 g_output (`e2e/grad`) with the stand-in detector and alignment network
The reference's crop is float32 by construction (its canvas is torch.zeros), so the float64 twin of every value comes
from this tool's restatement of the closed form, which is first asserted equal to the reference in float32.  The tool
prints the reference's float32 error against the twin for every recorded value: those figures, and the boxes, stand in
tests/landmark_cases.py, and the tool refuses to write when the table there disagrees with what it computes.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('FMGAN_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import landmark_cases as lc  # noqa: E402


def transform(point, center, scale, resolution, invert=False):
    """face_alignment.utils.transform, float32."""
    pt = torch.ones(3)
    pt[0], pt[1] = float(point[0]), float(point[1])
    h = 200.0 * torch.as_tensor(scale, dtype=torch.float32)
    center = torch.as_tensor(center, dtype=torch.float32)
    t = torch.eye(3)
    t[0, 0] = resolution / h
    t[1, 1] = resolution / h
    t[0, 2] = resolution * (-center[0] / h + 0.5)
    t[1, 2] = resolution * (-center[1] / h + 0.5)
    if invert:
        t = torch.inverse(t)
    return torch.matmul(t, pt)[0:2].int()


sys.modules.update(lc.stub_modules(transform=transform))
sys.path.insert(0, REF)
from Util import landmark_util as ref_lm  # noqa: E402
from Util import training_util as ref_tu  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'landmark.npz')


def npy(t):
    return t.detach().cpu().numpy()


def boxes_of(center_list, scale_list, r):
    rows = []
    for c, s in zip(center_list, scale_list):
        ul, br = transform([1, 1], c, s, r, True), transform([r, r], c, s, r, True)
        rows.append((int(ul[0]), int(ul[1]), int(br[0]), int(br[1])))
    return rows


def closed_form_crop(img, boxes, r):
    """The closed form of the crop in img's dtype: canvas[c, y, x] = (img[c, y + uy, x + ux] + 1) * 255 / 2 inside the
    image, 0 elsewhere, bilinear to r x r (align_corners=False), / 255."""
    n, c, h, w = img.shape
    scaled = (img + 1) * 255 / 2
    crops = []
    for i, (ux, uy, bx, by) in enumerate(boxes):
        canvas = torch.zeros((1, c, by - uy, bx - ux), dtype=img.dtype)
        y0, y1, x0, x1 = max(uy, 0), min(by, h), max(ux, 0), min(bx, w)
        canvas[..., y0 - uy:y1 - uy, x0 - ux:x1 - ux] = scaled[i:i + 1, :, y0:y1, x0:x1]
        crops.append(F.interpolate(canvas, (r, r), mode='bilinear', align_corners=False))
    return torch.cat(crops) / 255.0


def reference_crop(img, center_list, scale_list, r):
    """Get_HeatMap_PyTorch's lines around Crop_PyTorch (landmark_util.py:182, 189-196) for given centers and scales."""
    scaled = (img + 1) * 255 / 2
    crops = [ref_lm.Crop_PyTorch(scaled[i:i + 1], center_list[i], scale_list[i], r) for i in range(img.shape[0])]
    return torch.cat(crops) / 255.0


def err(a32, b64):
    return float((a32.double() - b64).abs().max())


def report(name, ref_err, value_range, table, key_err, key_range):
    print(f'{name}: reference fp32 error {ref_err:.3e}, range {value_range:.3e}, bound {lc.bound(ref_err, value_range):.3e}')
    ok = abs(table[key_err] - ref_err) <= 0.02 * ref_err and abs(table[key_range] - value_range) <= 0.02 * value_range
    if not ok:
        print(f'    tests/landmark_cases.py holds {key_err}={table[key_err]!r}, {key_range}={table[key_range]!r}: '
              f'write {key_err}={ref_err:.3e}, {key_range}={value_range:.3e}')
    return ok


def gen_crop(out):
    ok = True
    for name, c in lc.CROP_CASES.items():
        r, st = c['r'], c['stride']
        centers, scales = lc.crop_center_scale(name)
        boxes = boxes_of(centers, scales, r)
        if [tuple(b) for b in c['box']] != boxes:
            print(f'{name}: boxes {boxes}; tests/landmark_cases.py holds {c["box"]}')
            ok = False
        img = lc.crop_image(name).requires_grad_(True)
        go = lc.crop_grad(name)
        ref = reference_crop(img, centers, scales, r)
        ref_grad, = torch.autograd.grad(ref, img, go)
        mine = closed_form_crop(img, boxes, r)
        mine_grad, = torch.autograd.grad(mine, img, go)
        assert torch.equal(ref, mine) and torch.equal(ref_grad, mine_grad), f'{name}: the closed form is not the reference'
        img64 = lc.crop_image(name).double().requires_grad_(True)
        twin = closed_form_crop(img64, boxes, r)
        twin_grad, = torch.autograd.grad(twin, img64, go.double())
        ok &= report(f'{name} forward', err(ref, twin), float(twin.abs().max()), c, 'fwd_ref_err', 'fwd_range')
        ok &= report(f'{name} backward', err(ref_grad, twin_grad), float(twin_grad.abs().max()), c, 'bwd_ref_err', 'bwd_range')
        out[f'{name}/out'] = npy(ref)[:, :, ::st, ::st]
        out[f'{name}/grad'] = npy(ref_grad)[:, :, ::st, ::st]
    return ok


def gen_decode(out):
    ok = True
    for name, c in lc.DECODE_CASES.items():
        hm = lc.decode_maps(name)
        for seed in range(64):
            center, scale = lc.decode_center_scale(name, seed)
            preds, _ = ref_lm.Get_Preds_FromHeatMap_PyTorch(hm.clone(), 'cpu')
            h = 200.0 * scale.double().view(2, 1, 1)
            before = (preds.double() - 64 * (-center.double().view(2, 1, 2) / h + 0.5)) * h / 64
            if float((before - before.round()).abs().min()) >= 1e-3:
                break
        else:
            raise SystemExit(f'{name}: no seed keeps preds_orig away from the integers')
        if seed != c['cs_seed']:
            print(f'{name}: cs_seed must be {seed}; tests/landmark_cases.py holds {c["cs_seed"]}')
            ok = False
        preds, preds_orig = ref_lm.Get_Preds_FromHeatMap_PyTorch(hm.clone(), 'cpu', [center[0], center[1]],
                                                                 [float(scale[0]), float(scale[1])])
        assert torch.equal(preds_orig.double(), before.trunc()), f'{name}: the closed form of transform is not the reference'
        for m, want in enumerate(lc.decode_expected_preds(name)):
            assert want is None or tuple(preds[m // 5, m % 5].tolist()) == want, (name, m, preds[m // 5, m % 5], want)
        out[f'{name}/preds'], out[f'{name}/preds_orig'] = npy(preds), npy(preds_orig)
        print(f'{name}: preds_orig at least {float((before - before.round()).abs().min()):.2e} from an integer')
    return ok


def gen_distance(out):
    c = lc.DISTANCE_CASE
    a, b, g = lc.distance_inputs()
    a.requires_grad_(True)
    d = torch.sum(torch.square(a - b), dim=(1, 2, 3))                   # training_util.py:221 without its mean
    ga, = torch.autograd.grad(d, a, g)
    a64 = a.detach().double().requires_grad_(True)
    d64 = torch.sum(torch.square(a64 - b.double()), dim=(1, 2, 3))
    ga64, = torch.autograd.grad(d64, a64, g.double())
    ok = report('distance forward', err(d, d64), float(d64.abs().max()), c, 'out_ref_err', 'out_range')
    ok &= report('distance backward', err(ga, ga64), float(ga64.abs().max()), c, 'grad_ref_err', 'grad_range')
    out['dist/out'] = npy(d)
    out['dist/grad_a'] = npy(ga)[:, :, ::c['stride'], ::c['stride']]
    return ok


def twin_heatmap(img64, fa64, boxes, r=256):
    return fa64.face_alignment_net(closed_form_crop(img64, boxes, r))


def gen_e2e(out):
    c = lc.E2E
    fa = lc.Alignment()
    g_output, r_input = lc.e2e_images('g').requires_grad_(True), lc.e2e_images('r')
    ok = True
    with torch.no_grad():
        bboxes = ref_lm.Batch_Img_Face_Detection((g_output + 1) * 255 / 2, fa.face_detector, 'cpu')
        for which in ('g', 'r'):
            olist = fa.face_detector.face_detector(((lc.e2e_images(which) + 1) * 255 / 2).flip(-3)
                                                   - torch.tensor([104.0, 117.0, 123.0]).view(1, 3, 1, 1))
            for i in range(c['shape'][0]):
                cls, reg = F.softmax(olist[0], 1)[i:i + 1].numpy(), olist[1][i:i + 1].numpy()
                t = np.tanh(reg[0].reshape(4, -1).mean(1).astype(np.float64))
                raw = np.array([30 + 10 * t[0] - 14 - 8 * t[2], 32 + 10 * t[1] - 16 - 8 * t[3], 30 + 10 * t[0] + 14 + 8 * t[2],
                                32 + 10 * t[1] + 16 + 8 * t[3]])
                frac = np.abs(raw - np.floor(raw) - 0.5).min()
                score = float(cls[0, 1].mean())
                print(f'e2e {which} sample {i}: box before rounding {np.round(raw, 3)}, score {score:.3f}')
                assert frac > 0.02 and abs(score - 0.5) > 0.1, 'the stand-in detector\'s decision is not robust'
    got = [[float(v) for v in b[:4]] for b in bboxes]
    want = [[float(v) for v in b[:4]] for b in c['bbox']]
    if got != want:
        print(f'e2e: boxes {got}; tests/landmark_cases.py holds {want}')
        ok = False
    heatmap, center_list, scale_list = ref_lm.Get_HeatMap_PyTorch(g_output, fa, 'cpu')
    loss = ref_tu.Heat_Map_Loss(g_output, r_input, fa, 'cpu')
    grad, = torch.autograd.grad(loss, g_output)
    # float64 twin: the same boxes, the closed form, the stand-in network in float64
    fa64 = lc.Alignment(dtype=torch.float64)
    g64 = lc.e2e_images('g').double().requires_grad_(True)
    boxes_g = boxes_of(center_list, scale_list, 256)
    _, cl_r, sl_r = ref_lm.Get_HeatMap_PyTorch(r_input, fa, 'cpu')
    hm64 = twin_heatmap(g64, fa64, boxes_g)
    hm64_r = twin_heatmap(lc.e2e_images('r').double(), fa64, boxes_of(cl_r, sl_r, 256))
    loss64 = torch.mean(torch.sum(torch.square(hm64_r - hm64), dim=(1, 2, 3)))
    grad64, = torch.autograd.grad(loss64, g64)
    ok &= report('e2e heatmap', err(heatmap, hm64), float(hm64.abs().max()), c, 'hm_ref_err', 'hm_range')
    ok &= report('e2e loss', err(loss, loss64), float(loss64.abs()), c, 'loss_ref_err', 'loss_range')
    ok &= report('e2e grad', err(grad, grad64), float(grad64.abs().max()), c, 'grad_ref_err', 'grad_range')
    st = c['hm_stride']
    out['e2e/heatmap'] = npy(heatmap)[:, :, ::st, ::st]
    out['e2e/center'] = np.stack([npy(x) for x in center_list])
    out['e2e/scale'] = np.asarray(scale_list, dtype=np.float64)
    out['e2e/loss'] = npy(loss)
    out['e2e/grad'] = npy(grad)
    return ok


def main():
    out = {}
    ok = gen_crop(out)
    ok &= gen_decode(out)
    ok &= gen_distance(out)
    ok &= gen_e2e(out)
    if not ok:
        raise SystemExit('tests/landmark_cases.py disagrees with what the reference gives (see above): nothing written')
    np.savez_compressed(OUT, **out)
    print('landmark', len(out), os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
