#!/usr/bin/env python3
"""Face-regional loss (csrc/face_region.hip) against the reference's composite, on the GPU.

    python tools/bench_face_region.py [--iters N] [--json PATH]

Shapes: C=3 renders / images at 256^2 B=16 and 1024^2 B=8.  Per shape, median of N timed calls (HIP events):
  hip fwd kernel   fmgan_face_region_loss_f32 alone (partials preallocated)
  hip fwd op       op.face_region.face_region_loss forward (kernel + the two small partial sums)
  hip bwd kernel   fmgan_face_region_backward_f32 alone (output preallocated)
  hip fwd+bwd      the autograd Function: forward + backward
  ref fwd+bwd      the reference's composite (Util/training_util.py:228-256), restated: mean over channels, compare,
                   mask to a CPU float tensor and back, two masked products, difference, square, mean; autograd backward
Bytes: the forward reads r and g (2 x 4 x numel), the backward reads r, g and writes dg (3 x 4 x numel).  GB/s and the
share of the 8 TB/s HBM peak are given for the kernel-alone rows.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import torch  # noqa: E402

import ds_cases  # noqa: E402
import synth  # noqa: E402
from op import _native  # noqa: E402
from op.face_region import face_region_loss  # noqa: E402

HBM_PEAK_GBS = 8000.0
SHAPES = [(16, 3, 256, 256), (8, 3, 1024, 1024)]


def timeit(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def reference_composite(r, g):
    mask = (torch.mean(r, dim=1) > -1).type(torch.FloatTensor)        # a CPU tensor, as the reference's
    m = mask.unsqueeze(1).to(r.device)
    return torch.mean(torch.square(r * m - g * m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    d = torch.device('cuda', 0)
    L = _native.lib()
    rows = []
    for shape in SHAPES:
        b, c, h, w = shape
        n = b * c * h * w
        r = ds_cases.face_render('bench/r', shape).to(d)
        g = synth.tensor('bench/g', shape, dist='uniform').to(d).requires_grad_(True)
        gl = torch.ones((), device=d)
        partial = torch.empty((b, L.fmgan_face_region_blocks(b, h * w)), device=d)
        dg = torch.empty_like(g)
        stream = torch.cuda.current_stream(d).cuda_stream

        def fwd_kernel():
            _native.check(L.fmgan_face_region_loss_f32(r.data_ptr(), g.data_ptr(), partial.data_ptr(), b, c, h * w,
                                                       stream), 'face_region_loss')

        def bwd_kernel():
            _native.check(L.fmgan_face_region_backward_f32(r.data_ptr(), g.data_ptr(), gl.data_ptr(), dg.data_ptr(), b,
                                                           c, h * w, stream), 'face_region_backward')

        def fwd_op():
            with torch.no_grad():
                face_region_loss(r, g)

        def hip_both():
            g.grad = None
            face_region_loss(r, g).backward()

        def ref_both():
            g.grad = None
            reference_composite(r, g).backward()

        # same value on both sides before anything is timed
        lh, lr = float(face_region_loss(r, g).detach()), float(reference_composite(r, g).detach())
        row = dict(shape=list(shape), loss_hip=lh, loss_ref=lr, fwd_bytes=8 * n, bwd_bytes=12 * n)
        for name, fn in (('hip_fwd_kernel', fwd_kernel), ('hip_fwd_op', fwd_op), ('hip_bwd_kernel', bwd_kernel),
                         ('hip_fwd_bwd', hip_both), ('ref_fwd_bwd', ref_both)):
            med, mn = timeit(fn, a.iters)
            row[name + '_us'] = round(med, 2)
            row[name + '_us_min'] = round(mn, 2)
        for k, nbytes in (('hip_fwd_kernel', 8 * n), ('hip_bwd_kernel', 12 * n)):
            gbs = nbytes / (row[k + '_us'] * 1e-6) / 1e9
            row[k + '_gbs'] = round(gbs, 1)
            row[k + '_of_peak'] = round(gbs / HBM_PEAK_GBS, 3)
        row['speedup_fwd_bwd'] = round(row['ref_fwd_bwd_us'] / row['hip_fwd_bwd_us'], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
