#!/usr/bin/env python3
"""FID (Evaluation/fid.py) on the GPU: the two kernels against their composites, and the sampling loop against the
reference's structure.

    python tools/bench_fid.py [--rounds R] [--window S] [--md PATH] [--skip-loop] [--inception-error]

(a) feature statistics (op/fid_stats.py), one update of a [b, 2048] fp32 batch into float64 moments, b = 100 and 64:
      kernel     fmgan_fid_stats_update_f32 alone
      composite  the float64 torch form: y = feat.double() - shift; sum += y.sum(0); outer.addmm_(y.T, y)
    Bytes the update must move, computed from the shape: the upper half of `outer` (tiles on or above the diagonal) read
    and written once, plus feat, shift and sum.
(b) Inception input stage (op/inception_input.py), S = 256 and 1024 at B = 8 and 64, normalize_input on:
      kernel     fmgan_inception_input_f32 alone, output preallocated
      fused      op.inception_input.inception_input (kernel + allocation)
      composite  F.interpolate, 2x - 1, layout copy
(c) the sampling loop, N = 2000 at batch 100, Generator(256, 512, 8) with stored noise, InceptionV3() with its own
    initialisation (a load figure):
      fused      Sample_Statistics(fuse=True) + finish(): nothing leaves the device inside the loop
      reference  the reference's structure: module-by-module network behind F.interpolate, every batch's features to the
                 host, np.mean / np.cov of the concatenation at the end
--inception-error prints the figure tests/test_fid_gpu.py's MODULES_GPU_VS_F64 records: the module-by-module forward of
InceptionV3() (seed 0) at [2, 3, 256, 256] on the GPU against the same network in float64 on the CPU, and the folded, fused
forward against the module-by-module one on the GPU, each as max |diff| / max |out|.
Method: HIP events on the current stream round a window of n back-to-back calls, n chosen per version so that a window
lasts at least --window seconds (default 0.3; the loop: one call); every version is warmed up first; the versions
alternate inside each of R rounds; reported per call: the median round and the lowest / highest round.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
from op import _native, inception_input as II  # noqa: E402

HBM_PEAK_GBS = 8000.0


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def window_time(fn, n):
    """Microseconds per call over one window of n back-to-back calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / n


def alternate(versions, rounds, window_s, warm=3):
    """{name: (median round, lowest round, highest round, calls per window)}, microseconds per call."""
    calls = {}
    for name, fn in versions.items():
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        once = max(window_time(fn, 4), 1e-3)
        calls[name] = max(1, int(window_s * 1e6 / once) + 1)
    per_round = {k: [] for k in versions}
    for _ in range(rounds):
        for name, fn in versions.items():
            per_round[name].append(window_time(fn, calls[name]))
    return {k: (round(median(v), 2), round(min(v), 2), round(max(v), 2), calls[k]) for k, v in per_round.items()}


def fmt(t):
    return f'{t[0]} ({t[1]} .. {t[2]})'


def stats_rows(a, d):
    L = _native.lib()
    dim, rows = 2048, []
    for b in (100, 64):
        feat = torch.relu(synth.tensor('bench_fid/feat', (b, dim)) + 0.7).to(d)
        shift = feat.double().mean(0)
        total = torch.zeros(dim, dtype=torch.float64, device=d)
        outer = torch.zeros(dim, dim, dtype=torch.float64, device=d)
        total2, outer2 = torch.zeros_like(total), torch.zeros_like(outer)
        stream = torch.cuda.current_stream(d).cuda_stream

        def kernel():
            _native.check(L.fmgan_fid_stats_update_f32(feat.data_ptr(), shift.data_ptr(), total.data_ptr(),
                                                       outer.data_ptr(), b, dim, stream), 'fid_stats_update')

        def composite():
            y = feat.double() - shift
            total2.add_(y.sum(0))
            outer2.addmm_(y.T, y)

        t = alternate({'kernel': kernel, 'composite': composite}, a.rounds, a.window)
        tiles = (dim // 16) * (dim // 16 + 1) // 2
        must = 2 * tiles * 256 * 8 + b * dim * 4 + 3 * dim * 8
        gbs = must / t['kernel'][0] / 1e3
        rows.append(f"| [{b}, {dim}] | {fmt(t['kernel'])} | {gbs:.1f} ({gbs / HBM_PEAK_GBS:.3f}) of {must} B | "
                    f"{fmt(t['composite'])} | {t['composite'][0] / t['kernel'][0]:.2f} |")
        print(rows[-1], flush=True)
    return rows


def input_rows(a, d):
    L = _native.lib()
    rows = []
    for s in (256, 1024):
        for b in (8, 64):
            x = synth.tensor('bench_fid/x', (b, 3, s, s), dist='uniform').to(d)
            assert II.inception_input_serves(x)
            out = torch.empty((b, 3, 299, 299), device=d).contiguous(memory_format=torch.channels_last)
            stream = torch.cuda.current_stream(d).cuda_stream

            def kernel():
                _native.check(L.fmgan_inception_input_f32(x.data_ptr(), out.data_ptr(), b, s, s, 1, stream),
                              'inception_input')

            def fused():
                return II.inception_input(x)

            def composite():
                return II.inception_input_composite(x)

            ref = composite()
            diff = float((fused() - ref).abs().max())       # the gate of tests/test_fid_gpu.py with normalize_input
            assert diff <= 2.0 ** -21 * float(x.abs().max()) + 2 * 2.0 ** -24 * float(ref.abs().max()), diff
            del ref
            t = alternate({'kernel': kernel, 'fused': fused, 'composite': composite}, a.rounds, a.window)
            rows.append(f"| [{b}, 3, {s}, {s}] | {fmt(t['kernel'])} | {fmt(t['fused'])} | {fmt(t['composite'])} | "
                        f"{t['composite'][0] / t['fused'][0]:.2f} |")
            print(rows[-1], flush=True)
            del x, out
    return rows


def loop_rows(a, d):
    import fid_cases as fc
    import stylegan2
    from Evaluation import fid as FID
    from Evaluation.inception import InceptionV3
    n, batch = 2000, 100
    g = stylegan2.Generator(256, 512, 8)
    g.load_state_dict(synth.state_dict('generator', g.state_dict(), seed=4))
    gen = fc.Pinned(g.to(d).eval())
    torch.manual_seed(0)
    inc = InceptionV3().to(d).eval()
    latents = [torch.randn(batch, 512, device=d) for _ in range(n // batch)]

    def sampler(idx, b, dim, device):
        return latents[idx]

    def fused():
        stats = FID.Sample_Statistics(gen, inc, 1, None, batch, n, d, sampler=sampler, fuse=True)
        return tuple(t.cpu().numpy() for t in stats.finish())

    def reference():
        feats = []
        with torch.no_grad():
            for idx in range(n // batch):
                img = gen([latents[idx]], truncation=1, truncation_latent=None)
                feats.append(inc.forward_modules(img)[0].view(batch, -1).to('cpu'))
        feats = torch.cat(feats, 0).numpy()
        return np.mean(feats, 0), np.cov(feats, rowvar=False)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for fn in (fused, reference):          # warm-up: MIOpen's searches, the allocator
        print('warm-up', fn.__name__, round(wall(fn)[0], 1), 'ms', flush=True)
    times = {'fused': [], 'reference': []}
    for _ in range(a.rounds):
        for name, fn in (('fused', fused), ('reference', reference)):
            ms, out = wall(fn)
            times[name].append(ms)
            times[name + '_out'] = out
    (m1, c1), (m2, c2) = times['fused_out'], times['reference_out']
    rel = float(np.abs(c1 - c2).max() / np.abs(c2).max())
    row = lambda v: f'{median(v):.1f} ({min(v):.1f} .. {max(v):.1f})'      # noqa: E731
    rows = [f"| Generator(256), {n // batch} x {batch} | {row(times['fused'])} | {row(times['reference'])} | "
            f"{median(times['reference']) / median(times['fused']):.3f} | {rel:.2e} |"]
    print(rows[-1], flush=True)
    return rows


def inception_error(d):
    from Evaluation.inception import InceptionV3
    torch.manual_seed(0)
    m = InceptionV3().eval()
    x = (synth.tensor('fid_gpu/inception/x', (2, 3, 256, 256), dist='uniform') + 1) / 2
    with torch.no_grad():
        ref = m.double().forward_modules(x.double())[0]
        m = m.float().to(d)
        plain = m.forward_modules(x.to(d))[0]
        folded = m(x.to(d))[0]
    scale = float(ref.abs().max())
    print('inception-error: modules GPU vs CPU float64, max |diff| / max |out|:',
          float((plain.cpu().double() - ref).abs().max()) / scale)
    print('inception-error: folded + fused vs modules on the GPU:',
          float((folded - plain).abs().max()) / float(plain.abs().max()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--md')
    ap.add_argument('--skip-loop', action='store_true')
    ap.add_argument('--inception-error', action='store_true')
    a = ap.parse_args()
    d = torch.device('cuda', 0)
    if a.inception_error:
        inception_error(d)
        return
    cmd = 'python tools/bench_fid.py ' + ' '.join(sys.argv[1:])
    md = [f'# FID: feature statistics, Inception input stage and the sampling loop (`tools/bench_fid.py`)', '',
          f'One MI355X (the runtime\'s device name: {torch.cuda.get_device_name(0)}).  `{cmd.strip()}`.  HIP events round '
          f'windows of back-to-back calls of at least {a.window} s; every version warmed up; the versions alternate inside '
          f'each of {a.rounds} rounds.  Figures: µs per call (a, b) or ms of wall time per loop (c), median round (lowest .. '
          f'highest round).', '',
          '## (a) One update of the float64 moments, D = 2048', '',
          '| feat | `fmgan_fid_stats_update_f32`, µs | GB/s of the bytes it must move (share of 8 TB/s) | float64 torch '
          'composite, µs | composite ÷ kernel |', '|---|---|---|---|---|'] + stats_rows(a, d)
    md += ['', '## (b) Inception input stage, normalize_input on', '',
           '| image | `fmgan_inception_input_f32` alone, µs | `inception_input`, µs | `inception_input_composite`, µs | '
           'composite ÷ fused |', '|---|---|---|---|---|'] + input_rows(a, d)
    if not a.skip_loop:
        md += ['', '## (c) Sampling loop, N = 2000', '',
               '| generator, batches | fused (`Sample_Statistics` + `finish`), ms | reference structure, ms | reference ÷ '
               'fused | largest |cov difference| ÷ max |cov| |', '|---|---|---|---|---|'] + loop_rows(a, d)
    text = '\n'.join(md) + '\n'
    if a.md:
        with open(a.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
