"""The 16-bit activation kernels (csrc/act16.hip) against the fp32 path they replace, on the GPU (profiles/act16.md).

  kernels    act16_fba, act16_fba_bwd and ufd16_fir (bf16) stand-alone at the shapes of Discriminator(1024)'s first block at
             B = 8 ([8, 32, 1024, 1024] activations; the (2, 2)-padded 4 x 4 blur of the same tensor), next to their fp32
             siblings fba_f32_planes, fba_bwd_bias_f32 and ufd_rowmarch_f32 at the same shapes in the same run: device
             time per call from events around --calls calls after warm-up, bytes the op must move (inputs once, output
             once) over that time, and the share of the 8 TB/s HBM peak.
  d          Discriminator(--sizes) forward + backward of the logistic loss + the R1 step under torch.autocast(bfloat16),
             with _native.activation_io 'fp32' and '16' alternated in blocks, device time per iteration.
  trainstep  bench.py's trainstep1024 configuration (Generator(1024), Discriminator(1024), 18 styles, LPIPS + ArcFace,
             B = 8) in bf16 through Trainer.step with args.precision = 'bf16', bf16_io off and on, alternated in whole
             16-iteration windows (R1 every 16, path length every 4: a window holds the same mix of iterations).

Without --part the driver starts --procs fresh processes per part, one after the other, and reports medians and the
spread (max - min) over them; with --part it is one such process and prints one JSON line.  A measurement path that
finds no GPU fails.

    python tools/bench_act16.py [--parts kernels d trainstep] [--procs 3] [--out profiles/act16.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_TBS = 8.0


def say(*a):
    print(*a, flush=True)


def timed(fn, calls, warmup):
    """Device milliseconds per call of fn(): events around `calls` calls after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def part_kernels(a, device):
    from op import _native
    b, c, h, w = a.kernel_shape
    n = b * c * h * w
    res = {}
    x32 = torch.randn(b, c, h, w, device=device)
    bias = torch.randn(c, device=device)
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], device=device)
    k = torch.outer(k1, k1) / 64
    empty32 = x32.new_empty(0)
    for name, x in (('f32', x32), ('bf16', x32.bfloat16())):
        es = x.element_size()
        empty = x.new_empty(0)
        out = _native.fused_bias_act(x, bias, empty, 3, 0, 0.2, 2 ** 0.5)
        ms = timed(lambda: _native.fused_bias_act(x, bias, empty, 3, 0, 0.2, 2 ** 0.5), a.calls, a.warmup)
        res[f'fba_{name}'] = dict(ms=ms, bytes=2 * n * es)
        bwd = _native.fused_bias_act_backward if name == 'f32' else _native.fused_bias_act16_backward
        assert bwd(x, out, 0.2, 2 ** 0.5) is not None
        ms = timed(lambda: bwd(x, out, 0.2, 2 ** 0.5), a.calls, a.warmup)
        res[f'fba_bwd_{name}'] = dict(ms=ms, bytes=3 * n * es)
        del out
        x4 = x.reshape(-1, h, w, 1)
        y = _native.upfirdn2d(x4, k, 1, 1, 1, 1, 2, 2, 2, 2)
        ms = timed(lambda: _native.upfirdn2d(x4, k, 1, 1, 1, 1, 2, 2, 2, 2), a.calls, a.warmup)
        res[f'fir_{name}'] = dict(ms=ms, bytes=(n + y.numel()) * es)
        del y
    for r in res.values():
        r['tb_per_s'] = r['bytes'] / (r['ms'] * 1e-3) / 1e12
        r['share_of_hbm_peak'] = r['tb_per_s'] / HBM_PEAK_TBS
    return dict(shape=[b, c, h, w], calls=a.calls, kernels=res)


def d_iteration(D, opt, real, fake):
    """The D side of a training iteration: logistic loss + backward + step, then the R1 step (double backward)."""
    from Util.training_util import d_logistic_loss, d_r1_loss
    loss = d_logistic_loss(D(real), D(fake))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    real = real.detach().requires_grad_(True)
    r1 = d_r1_loss(D(real), real)
    opt.zero_grad(set_to_none=True)
    (10 / 2 * r1 * 16).backward()
    opt.step()


def part_d(a, device):
    import stylegan2
    from op import _native
    res = {}
    for size in a.sizes:
        batch = 8 if size >= 1024 else 16
        torch.manual_seed(size)
        D = stylegan2.Discriminator(size).to(device)
        opt = torch.optim.Adam(D.parameters(), lr=1e-4)
        real = torch.rand(batch, 3, size, size, device=device) * 2 - 1
        fake = torch.rand(batch, 3, size, size, device=device) * 2 - 1

        def run(mode):
            with torch.autocast('cuda', dtype=torch.bfloat16), _native.activation_io(mode):
                d_iteration(D, opt, real, fake)
        ms = {'fp32': [], '16': []}
        for mode in ms:
            timed(lambda: run(mode), 1, a.warmup)
        for _ in range(a.blocks):                 # alternate the two modes
            for mode in ms:
                ms[mode].append(timed(lambda: run(mode), a.iters, 0))
        res[str(size)] = dict(batch=batch, iters=a.iters, blocks=a.blocks,
                              ms_fp32=statistics.median(ms['fp32']), ms_16=statistics.median(ms['16']),
                              all_fp32=ms['fp32'], all_16=ms['16'])
    return res


def part_trainstep(a, device):
    import bench
    wl = bench.WORKLOADS['trainstep1024']
    nets = bench.build_models(wl['size'], device)
    _, tr = bench.make_trainstep(nets, wl['batch'], device, 0, 1, wl['size'], loss_nets=True)
    tr.args.precision = 'bf16'
    gen = torch.Generator(device='cpu').manual_seed(1234)
    photo = (torch.rand(wl['batch'], 3, 256, 256, generator=gen) * 2 - 1).to(device)
    render = (torch.rand(wl['batch'], 3, 256, 256, generator=gen) * 2 - 1).to(device)
    ref = (torch.rand(wl['batch'], 3, wl['size'], wl['size'], generator=gen) * 2 - 1).to(device)

    def window(io):
        tr.args.bf16_io = io
        for _ in range(16):
            tr.step(photo, render, ref)
    ms = {False: [], True: []}
    for io in ms:
        timed(lambda: window(io), 1, 0)           # warm-up: one whole window per mode
    for _ in range(a.windows):
        for io in ms:
            ms[io].append(timed(lambda: window(io), 1, 0) / 16)
    return dict(batch=wl['batch'], windows=a.windows, ms_per_iter_io_off=statistics.median(ms[False]),
                ms_per_iter_io_on=statistics.median(ms[True]), all_off=ms[False], all_on=ms[True])


PARTS = dict(kernels=part_kernels, d=part_d, trainstep=part_trainstep)


def spread(values):
    return dict(median=statistics.median(values), spread=max(values) - min(values), values=values)


def summarise(part, runs):
    if part == 'kernels':
        names = runs[0]['kernels']
        return {n: dict(ms=spread([r['kernels'][n]['ms'] for r in runs]),
                        tb_per_s=spread([r['kernels'][n]['tb_per_s'] for r in runs]),
                        share_of_hbm_peak=statistics.median([r['kernels'][n]['share_of_hbm_peak'] for r in runs]))
                for n in names}
    if part == 'd':
        return {s: dict(ms_fp32=spread([r[s]['ms_fp32'] for r in runs]), ms_16=spread([r[s]['ms_16'] for r in runs]))
                for s in runs[0]}
    return dict(ms_per_iter_io_off=spread([r['ms_per_iter_io_off'] for r in runs]),
                ms_per_iter_io_on=spread([r['ms_per_iter_io_on'] for r in runs]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--part', choices=sorted(PARTS), help='one measurement process (what the driver starts)')
    ap.add_argument('--parts', nargs='+', default=['kernels', 'd', 'trainstep'], choices=sorted(PARTS))
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--timeout', type=int, default=900, help='seconds per child process')
    ap.add_argument('--kernel-shape', type=int, nargs=4, default=[8, 32, 1024, 1024])
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--iters', type=int, default=4)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--windows', type=int, default=2)
    a = ap.parse_args()
    if a.part:
        if not torch.cuda.is_available():
            raise SystemExit('bench_act16: no GPU; nothing is measured without one')
        device = torch.device('cuda', 0)
        say(json.dumps({a.part: PARTS[a.part](a, device)}))
        return
    report = {}
    for part in a.parts:
        runs = []
        for i in range(a.procs):
            cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--calls', str(a.calls), '--warmup',
                   str(a.warmup), '--iters', str(a.iters), '--blocks', str(a.blocks), '--windows', str(a.windows),
                   '--kernel-shape'] + [str(v) for v in a.kernel_shape] + ['--sizes'] + [str(s) for s in a.sizes]
            pr = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
            if pr.returncode != 0:                # a failed child ends the measurement: nothing more is started
                raise SystemExit(f'bench_act16: {part} process {i} ended with status {pr.returncode}')
            runs.append(json.loads(pr.stdout.strip().split('\n')[-1])[part])
            say(f'{part} {i}:', json.dumps(runs[-1]))
        report[part] = dict(summary=summarise(part, runs), runs=runs)
        say(f'{part} summary:', json.dumps(report[part]['summary']))
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(report, f, indent=1)
    say(json.dumps({k: v['summary'] for k, v in report.items()}))


if __name__ == '__main__':
    main()
