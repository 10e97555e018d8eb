#!/usr/bin/env python3
"""Landmark stages on the GPU (op/landmark.py, Util/landmark_util.py) against the reference's structure.

    python tools/bench_landmark.py [--rounds R] [--window S] [--json PATH] [--md PATH]

The baseline is never the code under test: it is the reference's structure (Util/landmark_util.py, Util/training_util.py:
206-222, Evaluation/quant_eval.py:175-183) written here from aten ops:
  crop      per image: the scaled image to the host, a host canvas (torch.zeros), F.interpolate on the host, then the batch
            / 255 back to the device (Crop_PyTorch behind Get_HeatMap_PyTorch); forward, and forward + backward of <crop, g>
  decode    the B x 68 Python loop of _get_preds_fromhm_torch: two int() and four scalar reads per map, then transform()
            per point (torch.inverse of a 3 x 3 on the host)
  distance  torch.sum(torch.square(a - b), dim=(1, 2, 3)), forward, and forward + backward
Ours: op.landmark.face_crop / landmark_decode / heatmap_distance, and the kernels alone through the C ABI with preallocated
outputs, for which the bytes they must move are computed here from the shapes (crop: every image pixel inside a box read
once and the crop written; its backward: the crop's gradient read once and the image's written; distance: both inputs
read, backward also one gradient written) and divided by the time: achieved bandwidth, and its share of the HBM peak.
Shapes: [8, 3, 256, 256] and [16, 3, 256, 256] images, 256 x 256 crops, half the boxes the detector's fallback box and
half a face-sized one; heat maps [B, 68, 64, 64].
Edit-score batch: Evaluation.quant_eval.Get_Edit_Score on one [photo, render_1, render_2] batch of 8 with stand-in
generator functions, a stand-in detector and alignment network (tests/landmark_cases.py, 68 maps) and an fa_model,
against the reference's loop body restated with the baselines above; and the same call without an fa_model, for the cost
of the rest.
Also counted, per call, by the launch observer: our launches; and by a wrapper round torch.Tensor.cpu / .item / int():
the host synchronisations of either side.
Method: HIP events on the current stream round a window of n back-to-back calls, n chosen per version so that a window
lasts at least --window seconds; every version is warmed up first; the versions alternate inside each of R rounds; reported
per call: the median round and the lowest / highest round (tools/bench_ppl.py: alternate).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import landmark_cases as lc  # noqa: E402
import launches  # noqa: E402
import synth  # noqa: E402
from bench_ppl import alternate  # noqa: E402
from op import _native, landmark as L  # noqa: E402
from Util import landmark_util as LU  # noqa: E402

HBM_PEAK_GBS = 8000.0
BATCHES = (8, 16)
FACE_BBOX = [60.0, 70.0, 190.0, 215.0, 1.0]


# ----------------------------------------------------------------------------- the reference's structure, restated
def ref_crop(img, centers, scales, r=256):
    scaled = (img + 1) * 255 / 2
    crops = []
    for i in range(img.shape[0]):
        ul = LU.transform([1, 1], centers[i], scales[i], r, True)
        br = LU.transform([r, r], centers[i], scales[i], r, True)
        _, c, ht, wd = img.shape
        canvas = torch.zeros([1, c, int(br[1] - ul[1]), int(br[0] - ul[0])])
        nx = (max(1, -int(ul[0]) + 1), min(int(br[0]), wd) - int(ul[0]))
        ny = (max(1, -int(ul[1]) + 1), min(int(br[1]), ht) - int(ul[1]))
        ox = (max(1, int(ul[0]) + 1), min(int(br[0]), wd))
        oy = (max(1, int(ul[1]) + 1), min(int(br[1]), ht))
        canvas[..., ny[0] - 1:ny[1], nx[0] - 1:nx[1]] = scaled[i:i + 1, :, oy[0] - 1:oy[1], ox[0] - 1:ox[1]]
        crops.append(F.interpolate(canvas, (r, r), mode='bilinear'))
    return (torch.cat(crops) / 255.0).to(img.device)


def ref_decode(hm, centers, scales):
    b, c, h, w = hm.shape
    idx = torch.argmax(hm.reshape(b, c, h * w), axis=-1).float() + 1
    preds = idx.repeat_interleave(2).reshape(b, c, 2)
    preds[:, :, 0] = (preds[:, :, 0] - 1) % w + 1
    preds[:, :, 1] = torch.floor((preds[:, :, 1] - 1) / h) + 1
    for i in range(b):
        for j in range(c):
            hm_ = hm[i, j, :]
            px, py = int(preds[i, j, 0]) - 1, int(preds[i, j, 1]) - 1
            if 0 < px < 63 and 0 < py < 63:
                diff = torch.tensor([hm_[py, px + 1] - hm_[py, px - 1], hm_[py + 1, px] - hm_[py - 1, px]])
                preds[i, j] += (torch.sign(diff) * 0.25).to(hm.device)
    preds -= 0.5
    orig = torch.zeros_like(preds)
    for i in range(b):
        for j in range(c):
            orig[i, j] = LU.transform(preds[i, j], centers[i], scales[i], h, True)
    return preds, orig


def ref_distance(a, b):
    return torch.sum(torch.square(a - b), dim=(1, 2, 3))


def ref_detect(img, fa):
    x = ((img + 1) * 255 / 2).flip(-3) - torch.tensor([104.0, 117.0, 123.0], device=img.device).view(1, 3, 1, 1)
    olist = list(fa.face_detector.face_detector(x))
    for i in range(len(olist) // 2):
        olist[i * 2] = F.softmax(olist[i * 2], dim=1)
    olist = [o.data.cpu().numpy() for o in olist]
    boxes = []
    for i in range(img.shape[0]):
        bl = fa.face_detector._filter_bboxes(lc.standin_get_predictions([o[i:i + 1] for o in olist], 1)[0])
        bad = len(bl) == 0 or bl[0][0] < 0 or bl[0][1] < 0 or bl[0][2] > 255 or bl[0][3] > 255
        boxes.append(list(lc.FALLBACK_BBOX) if bad else bl[0])
    return boxes


def ref_heatmap_landmark(img, fa):
    pairs = [lc.box_center_scale([float(v) for v in b]) for b in ref_detect(img, fa)]
    centers, scales = [p[0] for p in pairs], [p[1] for p in pairs]
    hm = fa.face_alignment_net(ref_crop(img, centers, scales))
    return hm, ref_decode(hm, centers, scales)[1]


# ----------------------------------------------------------------------------- counting
class SyncCount:
    """Counts the device-to-host transfers made from Python inside the block, each of which waits for the stream:
    Tensor.cpu / .item / .tolist / __int__ / __float__ of a device tensor, and a device tensor assigned into a host
    tensor (the reference's canvas)."""
    NAMES = ('cpu', 'item', 'tolist', '__int__', '__float__')

    def __enter__(self):
        self.n, self.saved = 0, {}
        for name in self.NAMES + ('__setitem__',):
            orig = getattr(torch.Tensor, name)
            self.saved[name] = orig

            def wrapped(t, *a, _orig=orig, _set=name == '__setitem__', **k):
                if (torch.is_tensor(a[1]) and a[1].is_cuda and not t.is_cuda) if _set else t.is_cuda:
                    self.n += 1
                return _orig(t, *a, **k)
            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)
        return False


def counts(fn):
    with launches.observed() as rec, SyncCount() as sc:
        fn()
    return len(rec.names), sc.n


def boxes_for(b):
    pairs = [lc.box_center_scale(lc.FALLBACK_BBOX if i % 2 else FACE_BBOX) for i in range(b)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def gbs(nbytes, us):
    return round(nbytes / us / 1e3, 1)


def stage_rows(a, d):
    lib = _native.lib()
    rows = []
    for b in BATCHES:
        img = synth.tensor('bench_landmark/img', (b, 3, 256, 256), dist='uniform').to(d)
        g = synth.tensor('bench_landmark/g', (b, 3, 256, 256)).to(d)
        centers, scales = boxes_for(b)
        box = LU.Face_Crop_Boxes(centers, scales, 256)
        box_d = box.to(d)
        xg = img.clone().requires_grad_(True)
        out, grad = torch.empty_like(img), torch.empty_like(img)
        stream = torch.cuda.current_stream(d).cuda_stream
        assert L.face_crop_serves(img, 256)
        err = float((L.face_crop(img, box, 256) - ref_crop(img, centers, scales)).abs().max())
        assert err <= 1e-6, err
        inside = sum(max(0, min(by, 256) - max(uy, 0)) * max(0, min(bx, 256) - max(ux, 0)) for ux, uy, bx, by in box.tolist())
        fwd_bytes, bwd_bytes = 3 * 4 * (inside + b * 256 * 256), 3 * 4 * 2 * b * 256 * 256

        def k_fwd():
            _native.check(lib.fmgan_face_crop_fwd_f32(img.data_ptr(), box_d.data_ptr(), out.data_ptr(), b, 256, 256, 256,
                                                      stream), 'face_crop_fwd')

        def k_bwd():
            _native.check(lib.fmgan_face_crop_bwd_f32(g.data_ptr(), box_d.data_ptr(), grad.data_ptr(), b, 256, 256, 256,
                                                      stream), 'face_crop_bwd')
        versions = {
            'kernel fwd': k_fwd, 'kernel bwd': k_bwd,
            'ours fwd': lambda: L.face_crop(img, box, 256),
            'ours fwd+bwd': lambda: torch.autograd.grad((L.face_crop(xg, box, 256) * g).sum(), xg),
            'composite fwd': lambda: L.face_crop_composite(img, box, 256),
            'reference fwd': lambda: ref_crop(img, centers, scales),
            'reference fwd+bwd': lambda: torch.autograd.grad((ref_crop(xg, centers, scales) * g).sum(), xg),
        }
        t = alternate(versions, a.rounds, a.window)
        for name, v in t.items():
            row = dict(stage='crop', batch=b, version=name, us=v[0], lo=v[1], hi=v[2], calls=v[3])
            if name.startswith('kernel'):
                nb = fwd_bytes if name.endswith('fwd') else bwd_bytes
                row.update(bytes=nb, gbs=gbs(nb, v[0]), peak_share=round(gbs(nb, v[0]) / HBM_PEAK_GBS, 4))
            else:
                row['launches'], row['syncs'] = counts(versions[name])
            rows.append(row)
        # decode
        hm = synth.tensor('bench_landmark/hm', (b, 68, 64, 64)).to(d)
        want = ref_decode(hm, centers, scales)
        got = L.landmark_decode(hm, centers, scales)
        assert torch.equal(got[0], want[0]) and float((got[1] - want[1]).abs().max()) <= 1
        versions = {'ours': lambda: L.landmark_decode(hm, centers, scales),
                    'composite': lambda: L.landmark_decode_composite(hm, centers, scales),
                    'reference': lambda: ref_decode(hm, centers, scales)}
        t = alternate(versions, a.rounds, a.window)
        for name, v in t.items():
            n_l, n_s = counts(versions[name])
            rows.append(dict(stage='decode', batch=b, version=name, us=v[0], lo=v[1], hi=v[2], calls=v[3], launches=n_l,
                             syncs=n_s))
        # distance
        ha = synth.tensor('bench_landmark/ha', (b, 68, 64, 64)).to(d)
        hb = synth.tensor('bench_landmark/hb', (b, 68, 64, 64)).to(d).requires_grad_(True)
        m = 68 * 64 * 64
        partial = torch.empty((b, lib.fmgan_heatmap_distance_blocks(b, m)), device=d)
        gb, up = torch.empty_like(ha), torch.ones(b, device=d)

        def kd_fwd():
            _native.check(lib.fmgan_heatmap_distance_fwd_f32(ha.data_ptr(), hb.data_ptr(), partial.data_ptr(), b, m, stream),
                          'heatmap_distance_fwd')

        def kd_bwd():
            _native.check(lib.fmgan_heatmap_distance_bwd_f32(ha.data_ptr(), hb.data_ptr(), up.data_ptr(), None, gb.data_ptr(),
                                                             b, m, stream), 'heatmap_distance_bwd')
        versions = {'kernel fwd': kd_fwd, 'kernel bwd': kd_bwd,
                    'ours fwd': lambda: L.heatmap_distance(ha, hb.detach()),
                    'ours fwd+bwd': lambda: torch.autograd.grad(L.heatmap_distance(ha, hb).mean(), hb),
                    'reference fwd': lambda: ref_distance(ha, hb.detach()),
                    'reference fwd+bwd': lambda: torch.autograd.grad(ref_distance(ha, hb).mean(), hb)}
        t = alternate(versions, a.rounds, a.window)
        for name, v in t.items():
            row = dict(stage='distance', batch=b, version=name, us=v[0], lo=v[1], hi=v[2], calls=v[3])
            if name.startswith('kernel'):
                nb = b * m * 4 * (2 if name.endswith('fwd') else 3)
                row.update(bytes=nb, gbs=gbs(nb, v[0]), peak_share=round(gbs(nb, v[0]) / HBM_PEAK_GBS, 4))
            else:
                row['launches'], row['syncs'] = counts(versions[name])
            rows.append(row)
    return rows


def edit_rows(a, d):
    from Evaluation import quant_eval as QE
    sys.modules.update(lc.stub_modules())
    code = lambda p: 0.5 * p.mean((2, 3), keepdim=True)                       # noqa: E731
    QE.Encode_Photo = lambda p, e_tsr, e_wp, tsr_encode='Photo Image': code(p)
    QE.Forward_Inference_Reanimate = lambda c, r, *x, **k: c + 0.25 * r
    fa = lc.Alignment(d)
    fa.face_alignment_net = lc.AlignmentNet(68).to(d).requires_grad_(False).eval()

    class Face(torch.nn.Module):
        def forward(self, x):
            return F.adaptive_avg_pool2d(x, (2, 3)).reshape(x.shape[0], 6) + 0.1
    b = 8
    shift = torch.tensor([0.2, -0.6, 0.8, 0.0] * (b // 4)).view(b, 1, 1, 1)
    mk = lambda tag: (synth.tensor(f'bench_landmark/{tag}', (b, 3, 256, 256), dist='uniform', scale=0.2) + shift).to(d)  # noqa: E731
    loader = [[mk('p'), mk('r1'), mk('r2')]]

    def ours():
        return QE.Get_Edit_Score(loader, d, (None,) * 4, (Face(), None, fa))

    def rest():
        return QE.Get_Edit_Score(loader, d, (None,) * 4, (Face(), None, None))

    def reference():
        hmap, lmark = [], []
        with torch.no_grad():
            p = loader[0][0]
            for r in loader[0][1:]:
                g_out = code(p) + 0.25 * r
                hm_g, lm_g = ref_heatmap_landmark(g_out, fa)
                hm_r, lm_r = ref_heatmap_landmark(r, fa)
                hmap += ref_distance(hm_r, hm_g).cpu().tolist()
                lmark += np.mean(np.square((lm_r - lm_g).cpu().numpy()), axis=(1, 2)).tolist()
        return np.mean(hmap), np.mean(lmark)
    o, r = ours(), reference()
    assert abs(o[2] - r[0]) <= 1e-4 * abs(r[0]), (o, r)
    versions = {'ours (Get_Edit_Score with fa_model)': ours, 'Get_Edit_Score without fa_model': rest,
                'reference loop body (heat maps and landmarks only)': reference}
    t = alternate(versions, a.rounds, a.window)
    rows = []
    for name, v in t.items():
        n_l, n_s = counts(versions[name])
        rows.append(dict(stage='edit score', batch=b, version=name, us=v[0], lo=v[1], hi=v[2], calls=v[3], launches=n_l,
                         syncs=n_s))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_landmark.py measures on the GPU; there is no CPU fallback'
    d = torch.device('cuda', 0)
    rows = stage_rows(a, d) + edit_rows(a, d)
    lines = ['| stage | batch | version | us / call (median) | lowest | highest | launches | host syncs | GB/s | of HBM peak |',
             '|---|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append(f"| {r['stage']} | {r['batch']} | {r['version']} | {r['us']} | {r['lo']} | {r['hi']} | "
                     f"{r.get('launches', '')} | {r.get('syncs', '')} | {r.get('gbs', '')} | {r.get('peak_share', '')} |")
    text = '\n'.join(lines)
    print(text)
    if a.json:
        json.dump(dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, window=a.window, rows=rows), open(a.json, 'w'),
                  indent=1)
    if a.md:
        open(a.md, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
