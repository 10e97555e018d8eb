#!/usr/bin/env python3
"""LPIPS distance of one VGG tap (csrc/lpips_distance.hip) against the aten composite of lpips/__init__.py, on the GPU.

    python tools/bench_lpips_distance.py [--iters N] [--json PATH] [--md PATH]

Shapes: the five taps of BASELINE config 5 (1024^2 images, B = 8) and of the 256^2 training step (B = 16), float32,
NHWC-dense, f1 (the generated image's features) wanting a gradient as in the G step.  Per shape, after warm-up, the four
forms are timed in turn inside one loop (HIP events, median of N):
  fused fwd / composite fwd           forward only, no graph
  fused fwd+bwd / composite fwd+bwd   forward with a graph, then backward to grad_f1
and the two kernels alone (outputs preallocated).  Bytes: S = 4*N*C*H*W per feature; the forward must read 2 S, the
backward read 2 S and write 1 S.  GB/s and the share of the 8 TB/s HBM peak are given for the kernel-alone rows.
Memory: torch.cuda.max_memory_allocated over forward + backward, less what was allocated before (the inputs).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402

from op import _native  # noqa: E402
from op.lpips_distance import lpips_distance, lpips_distance_composite, lpips_distance_serves  # noqa: E402

HBM_PEAK_GBS = 8000.0
SHAPES = [(8, 64, 1024, 1024), (8, 128, 512, 512), (8, 256, 256, 256), (8, 512, 128, 128), (8, 512, 64, 64),
          (16, 64, 256, 256), (16, 128, 128, 128), (16, 256, 64, 64), (16, 512, 32, 32), (16, 512, 16, 16)]


def feature(shape, gen, d):
    n, c, h, w = shape
    t = torch.empty((n, h, w, c), device=d).normal_(generator=gen).add_(0.3).relu_()
    return t.permute(0, 3, 1, 2)


def timed(fn, s, e):
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3


def peak_extra(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    d = torch.device('cuda', 0)
    L = _native.lib()
    gen = torch.Generator(device=d).manual_seed(7)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = []
    for shape in SHAPES:
        n, c, h, w = shape
        hw, S = h * w, 4 * n * c * h * w
        f0, f1 = feature(shape, gen, d), feature(shape, gen, d).requires_grad_(True)
        wt = torch.rand((1, c, 1, 1), device=d, generator=gen)
        up = torch.ones((n, 1, 1, 1), device=d)
        assert lpips_distance_serves(f0, f1, wt)
        partial = torch.empty((n, L.fmgan_lpips_distance_blocks(n, c, hw)), device=d)
        g1 = torch.empty_like(f1)
        stream = torch.cuda.current_stream(d).cuda_stream
        f1d = f1.detach()

        def k_fwd():
            _native.check(L.fmgan_lpips_distance_f32(f0.data_ptr(), f1d.data_ptr(), wt.data_ptr(), partial.data_ptr(),
                                                     n, c, hw, 1e-10, stream), 'lpips_distance')

        def k_bwd():
            _native.check(L.fmgan_lpips_distance_backward_f32(f0.data_ptr(), f1d.data_ptr(), wt.data_ptr(),
                                                              up.data_ptr(), None, g1.data_ptr(), n, c, hw, 1e-10,
                                                              stream), 'lpips_distance_backward')

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(f0, f1, wt)
            return run

        def both(fn):
            def run():
                f1.grad = None
                fn(f0, f1, wt).backward(up)
            return run

        forms = {'kernel_fwd': k_fwd, 'kernel_bwd': k_bwd, 'fused_fwd': fwd(lpips_distance),
                 'composite_fwd': fwd(lpips_distance_composite), 'fused_fwd_bwd': both(lpips_distance),
                 'composite_fwd_bwd': both(lpips_distance_composite)}
        with torch.no_grad():                                   # same value on both sides before anything is timed
            dh, dr = lpips_distance(f0, f1, wt), lpips_distance_composite(f0, f1, wt)
        row = dict(shape=list(shape), feature_bytes=S, d_fused=float(dh[0]), d_composite=float(dr[0]))
        for fn in forms.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in forms}
        for _ in range(a.iters):
            for k, fn in forms.items():
                ts[k].append(timed(fn, s, e))
        for k, v in ts.items():
            v.sort()
            row[k + '_us'], row[k + '_us_min'] = round(v[len(v) // 2], 1), round(v[0], 1)
        for k, nbytes in (('kernel_fwd', 2 * S), ('kernel_bwd', 3 * S)):
            gbs = nbytes / (row[k + '_us'] * 1e-6) / 1e9
            row[k + '_gbs'], row[k + '_of_peak'] = round(gbs, 1), round(gbs / HBM_PEAK_GBS, 3)
        f1.grad = None
        row['fused_peak_extra_gb'] = round(peak_extra(forms['fused_fwd_bwd']) / 1e9, 3)
        f1.grad = None
        row['composite_peak_extra_gb'] = round(peak_extra(forms['composite_fwd_bwd']) / 1e9, 3)
        row['speedup_fwd'] = round(row['composite_fwd_us'] / row['fused_fwd_us'], 2)
        row['speedup_fwd_bwd'] = round(row['composite_fwd_bwd_us'] / row['fused_fwd_bwd_us'], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del f0, f1, f1d, g1, partial, forms
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rows=rows), f, indent=1)
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, 'w') as f:
            f.write('| shape (N,C,H,W) | S MB | kernel fwd us (GB/s, of 8 TB/s) | kernel bwd us (GB/s, of 8 TB/s) | fwd fused / composite us '
                    '| fwd+bwd fused / composite us | speed-up fwd+bwd | peak extra GB fused / composite |\n')
            f.write('|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write(f"| {tuple(r['shape'])} | {r['feature_bytes'] / 1e6:.1f} "
                        f"| {r['kernel_fwd_us']} ({r['kernel_fwd_gbs']}, {r['kernel_fwd_of_peak']:.0%}) "
                        f"| {r['kernel_bwd_us']} ({r['kernel_bwd_gbs']}, {r['kernel_bwd_of_peak']:.0%}) "
                        f"| {r['fused_fwd_us']} / {r['composite_fwd_us']} "
                        f"| {r['fused_fwd_bwd_us']} / {r['composite_fwd_bwd_us']} | {r['speedup_fwd_bwd']}x "
                        f"| {r['fused_peak_extra_gb']} / {r['composite_peak_extra_gb']} |\n")


if __name__ == '__main__':
    main()
