#!/usr/bin/env python3
"""Perceptual path length (Evaluation/ppl.py) on the GPU: the fused LPIPS input stage against the composite, and
PPL_Distances with the fused against the composite input stage.

    python tools/bench_ppl.py [--rounds R] [--window S] [--json PATH] [--previous PATH] [--md PATH] [--skip-loops]

(a) input stage alone (op/ppl_input.py), shift / scale of lpips.ScalingLayer:
      [16, 3, 1024, 1024]          f = 4, whole image
      [16, 3, 1024, 1024], crop    f = 2, window (384, 256, 512, 512)
      [128, 3, 256, 256]           f = 1
      kernel     fmgan_lpips_pair_input_f32 alone, outputs preallocated
      fused      op.ppl_input.pair_input (kernel + the two allocations)
      composite  op.ppl_input.pair_input_composite (slice, F.interpolate, two ScalingLayer calls, two layout copies)
    Bytes the stage must move, computed here from the shape: every output once, and the source rows that carry a tap,
    whole inside the window (memory moves lines, not taps: at f = 4 the taps are a quarter of the window's pixels and sit
    in half of its rows; at f = 1 and 2 every pixel of the window is a tap).  `tap_bytes` counts the taps alone.
(b) PPL_Distances, `fuse` on against off, real lpips.PerceptualLoss in channels_last, stored noise:
      Generator(256, 512, 8), 4 batches of 64 pairs;  Generator(1024, 512, 8), 4 batches of 8 pairs
Method: HIP events on the current stream round a window of n back-to-back calls, n chosen per version so that a window
lasts at least --window seconds (default 0.5); every version of a shape is warmed up first; the versions alternate inside
each of R rounds; reported per call: the median round and the lowest / highest round.  --previous names the JSON of an
earlier run of the same command: --md then writes both runs side by side, which shows the spread between processes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import torch  # noqa: E402

import synth  # noqa: E402
from op import _native, ppl_input  # noqa: E402

HBM_PEAK_GBS = 8000.0
STAGE_SHAPES = [((16, 3, 1024, 1024), False), ((16, 3, 1024, 1024), True), ((128, 3, 256, 256), False)]
LOOPS = [(256, 64, 4), (1024, 8, 4)]          # generator size, pairs per batch, batches


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


def stage_bytes(shape, window, f):
    n, _, h, w = shape
    y0, x0, hc, wc = window
    oh, ow = hc // f, wc // f
    out = n * 3 * oh * ow * 4
    tap_rows = (1 if f == 1 else 2) * oh                       # source rows of the window that carry a tap
    taps = (1 if f == 1 else 4) * oh * ow
    return n * 3 * tap_rows * wc * 4 + out, n * 3 * taps * 4 + out


def stage_rows(a, d):
    import lpips
    L = _native.lib()
    sl = lpips.ScalingLayer().to(d)
    rows = []
    for shape, crop in STAGE_SHAPES:
        x = synth.tensor('bench_ppl/x', shape, dist='uniform').to(d)
        assert ppl_input.pair_input_serves(x, crop)
        window, f = ppl_input.pair_input_plan(shape, crop)
        y0, x0, hc, wc = window
        n, _, h, w = shape
        out0 = torch.empty((n // 2, 3, hc // f, wc // f), device=d).contiguous(memory_format=torch.channels_last)
        out1 = torch.empty_like(out0)
        stream = torch.cuda.current_stream(d).cuda_stream
        shift, scale = sl.shift, sl.scale

        def kernel():
            _native.check(L.fmgan_lpips_pair_input_f32(x.data_ptr(), shift.data_ptr(), scale.data_ptr(), out0.data_ptr(),
                                                       out1.data_ptr(), n // 2, h, w, y0, x0, hc, wc, f, stream),
                          'lpips_pair_input')

        def fused():
            return ppl_input.pair_input(x, sl, crop=crop)

        def composite():
            return ppl_input.pair_input_composite(x, sl, crop=crop)

        got, want = fused(), composite()
        # the ScalingLayer's division may differ from the correctly rounded quotient in the last bit; the reduction's
        # association in the last bit of a value <= max|x|: a few ulp of max|x| / min scale
        gate = 8 * 2.0 ** -24 * float(x.abs().max() + 0.2) / 0.448
        for g, w_ in zip(got, want):
            assert tuple(g.shape) == tuple(w_.shape) and float((g - w_).abs().max()) <= gate
        t = alternate(dict(kernel=kernel, fused=fused, composite=composite), a.rounds, a.window)
        row_bytes, tap_bytes = stage_bytes(shape, window, f)
        gbs = row_bytes / (t['kernel'][0] * 1e-6) / 1e9
        row = dict(what='stage', shape=list(shape), crop=crop, window=list(window), f=f, bytes=row_bytes,
                   tap_bytes=tap_bytes, kernel_us=t['kernel'], fused_us=t['fused'], composite_us=t['composite'],
                   kernel_gbs=round(gbs, 1), kernel_of_peak=round(gbs / HBM_PEAK_GBS, 3),
                   kernel_tap_gbs=round(tap_bytes / (t['kernel'][0] * 1e-6) / 1e9, 1),
                   composite_over_fused=round(t['composite'][0] / t['fused'][0], 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


class PinNoise(torch.nn.Module):
    """The generator with its stored noise (randomize_noise=False); `.module` is where PPL_Distances finds `style`."""

    def __init__(self, g):
        super().__init__()
        self.module = g

    def forward(self, **kw):
        return self.module(randomize_noise=False, **kw)


def loop_rows(a, d):
    import lpips
    import stylegan2
    from Evaluation import ppl as P
    percept = lpips.PerceptualLoss(model='net-lin', net='vgg').to(d).to(memory_format=torch.channels_last)
    rows = []
    for size, batch, batches in LOOPS:
        g = stylegan2.Generator(size, 512, 8)
        g.load_state_dict(synth.state_dict('generator', g.state_dict(), seed=4))
        gen = PinNoise(g.to(d).eval().requires_grad_(False))

        def sampler(idx, b, dim, device):
            return (synth.tensor(f'bench_ppl/z/{idx}', (2 * b, dim)).to(device),
                    (synth.tensor(f'bench_ppl/t/{idx}', (b,), dist='uniform').to(device) + 1) / 2)
        zs = [sampler(i, batch, 512, d) for i in range(batches)]

        def run(fuse):
            def f():
                return P.PPL_Distances(gen, percept, batch * batches, batch, 1e-2, 512, d,
                                       sampler=lambda i, b, dim, dev_: zs[i], fuse=fuse)
            return f
        on, off = run(True), run(False)
        t = alternate(dict(fused=on, composite=off), a.rounds, a.window, warm=2)
        d_on, d_off = on(), off()
        row = dict(what='loop', generator=size, pairs_per_batch=batch, batches=batches, fused_us=t['fused'],
                   composite_us=t['composite'], composite_over_fused=round(t['composite'][0] / t['fused'][0], 4),
                   score_fused=float(P.PPL_Filter(d_on)), score_composite=float(P.PPL_Filter(d_off)),
                   max_rel_difference=float(((d_on - d_off).abs() / d_off.abs()).max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del g, gen
        torch.cuda.empty_cache()
    return rows


def _t(v):
    return f'{v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})'


def _ms(v):
    return f'{v[0] / 1e3:.2f} ({v[1] / 1e3:.2f} .. {v[2] / 1e3:.2f})'


def markdown(runs):
    """profiles/ppl.md from one or two runs of this command (dicts as written by --json)."""
    out = ['# Perceptual path length: LPIPS input stage and `PPL_Distances` (`tools/bench_ppl.py`)', '']
    r0 = runs[0]
    out += [f"One {r0['device']}, fp32.  `python tools/bench_ppl.py --json A.json`, then the same command again with "
            f"`--previous A.json --md profiles/ppl.md`: {len(runs)} run(s) of the same command in separate processes, "
            f"shown one row each.  HIP events round windows of back-to-back calls of at least {r0['window']} s; every "
            f"version warmed up; the versions alternate inside each of {r0['rounds']} rounds.  Figures: µs (stage) or ms "
            f"(loop) per call, median round (lowest .. highest round).", '',
            '## (a) Input stage alone', '',
            '| shape, window, f | run | `fmgan_lpips_pair_input_f32` alone, µs | GB/s of the bytes it must move (share of '
            '8 TB/s); taps alone | `pair_input`, µs | `pair_input_composite`, µs | composite ÷ fused |',
            '|---|---|---|---|---|---|---|']
    for i, row in enumerate(r0['rows']):
        if row['what'] != 'stage':
            continue
        for k, run in enumerate(runs):
            r = run['rows'][i]
            label = f"{r['shape']}, {tuple(r['window'])}, {r['f']}" if k == 0 else ''
            out.append(f"| {label} | {k + 1} | {_t(r['kernel_us'])} | {r['kernel_gbs']} ({r['kernel_of_peak']}) of "
                       f"{r['bytes']} B; {r['kernel_tap_gbs']} of {r['tap_bytes']} B | {_t(r['fused_us'])} | "
                       f"{_t(r['composite_us'])} | {r['composite_over_fused']} |")
    out += ['', '## (b) `PPL_Distances`, fused against composite input stage', '',
            '| generator, batches × pairs | run | fused, ms | composite, ms | composite ÷ fused | largest relative '
            'difference of a distance |', '|---|---|---|---|---|---|']
    for i, row in enumerate(r0['rows']):
        if row['what'] != 'loop':
            continue
        for k, run in enumerate(runs):
            r = run['rows'][i]
            label = f"Generator({r['generator']}), {r['batches']} × {r['pairs_per_batch']}" if k == 0 else ''
            out.append(f"| {label} | {k + 1} | {_ms(r['fused_us'])} | {_ms(r['composite_us'])} | "
                       f"{r['composite_over_fused']} | {r['max_rel_difference']:.2e} |")
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--previous', default=None)
    ap.add_argument('--md', default=None)
    ap.add_argument('--skip-loops', action='store_true')
    a = ap.parse_args()
    d = torch.device('cuda', 0)
    with torch.no_grad():
        rows = stage_rows(a, d)
        if not a.skip_loops:
            rows += loop_rows(a, d)
    this = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, window=a.window, rows=rows)
    for path, text in ((a.json, json.dumps(this, indent=1)),
                       (a.md, markdown(([json.load(open(a.previous))] if a.previous else []) + [this]))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                f.write(text)


if __name__ == '__main__':
    main()
