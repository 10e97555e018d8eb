#!/usr/bin/env python3
"""Image projection (Evaluation/image_projection) on the GPU: the fused image stage of the criterion against the
composite, one Adam iteration of the projection loop fused against unfused and with against without the cached target
features, and the run-to-run difference of the test trajectories.

    python tools/bench_projection.py [--rounds R] [--window S] [--json PATH] [--md PATH] [--skip-loops] [--skip-repeat]

(a) stage forward + backward (op/projection_loss.py), mask none, y wanted, shift / scale of lpips.ScalingLayer:
      [1, 3, 1024, 1024], [4, 3, 1024, 1024]   f = 4;    [8, 3, 256, 256]   f = 1
      kernel     fmgan_projection_loss_fwd_f32 + fmgan_projection_loss_bwd_f32 alone, outputs preallocated
      fused      op.projection_loss.projection_stage and autograd's backward of 0.5 * sq_sum + <y, g>
      composite  op.projection_loss.projection_stage_composite and the same backward
    Bytes the two kernels must move, computed here from the shape: forward x and target once (8 B per element) and y
    (12 B per reduced pixel); backward x, target and grad_x (12 B per element) and g_y (12 B per reduced pixel).
(b) one Adam iteration of the projection loop (Generator forward, criterion 'mse+lpips', backward, Adam step on W and the
    noise maps), real lpips.PerceptualLoss in channels_last:  Generator(1024, 512, 8) B = 1;  Generator(256, 512, 8) B = 4
      fused / unfused    project.PROJECT_FUSE on / off, target features cached
      cached / uncached  pre_cache on / off (off: the target goes through the trunk in every iteration), fused
(c) the trajectories of tests/projection_cases.py run twice in this process: the relative L2 difference between the two
    runs' displacements of W and of every noise map (MIOpen's trunk is not reproducible call to call).  Twice the largest
    figure is the floor of tests/test_projection_gpu.py's displacement gate.
Method: HIP events on the current stream round a window of n back-to-back calls, n chosen per version so that a window
lasts at least --window seconds (default 0.5); every version of a shape is warmed up first; the versions alternate inside
each of R rounds; reported per call: the median round and the lowest / highest round.
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
from bench_ppl import alternate  # noqa: E402
from op import _native, projection_loss as PL  # noqa: E402

HBM_PEAK_GBS = 8000.0
STAGE_SHAPES = [(1, 3, 1024, 1024), (4, 3, 1024, 1024), (8, 3, 256, 256)]
LOOPS = [(1024, 1), (256, 4)]          # generator size, batch


def stage_rows(a, d):
    import lpips
    L = _native.lib()
    sl = lpips.ScalingLayer().to(d)
    shift, scale = sl.shift.reshape(3), sl.scale.reshape(3)
    rows = []
    for shape in STAGE_SHAPES:
        b, _, s, _ = shape
        f = s // 256
        x = synth.tensor('bench_projection/x', shape, dist='uniform').to(d) * 1.2
        t = synth.tensor('bench_projection/t', shape, dist='uniform').to(d)
        g = synth.tensor('bench_projection/g', (b, 3, 256, 256)).to(d).contiguous(memory_format=torch.channels_last)
        assert PL.projection_stage_serves(x, t, None, sl)
        partial = torch.empty(L.fmgan_projection_loss_blocks(b, s, s, f), device=d)
        y = torch.empty((b, 256, 256, 3), device=d)
        grad = torch.empty_like(x)
        k = torch.ones(1, device=d)
        stream = torch.cuda.current_stream(d).cuda_stream
        xg = x.clone().requires_grad_(True)

        def kernel():
            _native.check(L.fmgan_projection_loss_fwd_f32(x.data_ptr(), t.data_ptr(), None, shift.data_ptr(),
                                                          scale.data_ptr(), partial.data_ptr(), y.data_ptr(), b, s, s, f,
                                                          stream), 'projection_loss_fwd')
            _native.check(L.fmgan_projection_loss_bwd_f32(x.data_ptr(), t.data_ptr(), None, g.data_ptr(), k.data_ptr(),
                                                          scale.data_ptr(), grad.data_ptr(), b, s, s, f, stream),
                          'projection_loss_bwd')

        def through(stage):
            def run():
                sq, ys = stage(xg, t, None, sl, True)
                return torch.autograd.grad(0.5 * sq + (ys * g).sum(), xg)[0]
            return run
        fused, composite = through(PL.projection_stage), through(PL.projection_stage_composite)
        got, want = fused(), composite()
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
        tm = alternate(dict(kernel=kernel, fused=fused, composite=composite), a.rounds, a.window)
        n, r = b * 3 * s * s, b * 256 * 256
        nbytes = 8 * n + 12 * r + 12 * n + 12 * r
        gbs = nbytes / (tm['kernel'][0] * 1e-6) / 1e9
        row = dict(what='stage', shape=list(shape), f=f, bytes=nbytes, kernel_us=tm['kernel'], fused_us=tm['fused'],
                   composite_us=tm['composite'], kernel_tbs=round(gbs / 1e3, 2),
                   kernel_of_peak=round(gbs / HBM_PEAK_GBS, 3),
                   composite_over_fused=round(tm['composite'][0] / tm['fused'][0], 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def loop_rows(a, d):
    import lpips
    import stylegan2
    from Evaluation.image_projection import project
    percept = lpips.PerceptualLoss(model='net-lin', net='vgg').to(d).to(memory_format=torch.channels_last)
    rows = []
    for size, batch in LOOPS:
        g = stylegan2.Generator(size, 512, 8)
        g.load_state_dict(synth.state_dict('generator', g.state_dict(), seed=4))
        g = g.to(d).eval().requires_grad_(False)
        target = 0.9 * synth.tensor('bench_projection/target', (batch, 3, size, size), dist='uniform').to(d)

        def iteration(fuse, cache):
            w = g.mean_latent(64).repeat(batch, 1).detach().requires_grad_(True)
            noises = [n.requires_grad_(True) for n in g.make_noise()]
            crit = project.ImageReconstructionLoss(device=d, loss='mse+lpips', pre_cache=cache, percept=percept)
            opt = torch.optim.Adam([w] + noises, lr=0.01)
            kwargs = {'noise_z': None, 'input_is_latent': True, 'latent_styles': [w], 'noise': noises}

            def run():
                project.PROJECT_FUSE = fuse
                opt.zero_grad()
                loss = crit(g(**kwargs), {'target': target, 'mask': None})
                loss.backward()
                opt.step()
                return loss
            return run
        versions = dict(fused=iteration(True, True), unfused=iteration(False, True), uncached=iteration(True, False))
        tm = alternate(versions, a.rounds, a.window, warm=2)
        project.PROJECT_FUSE = True
        row = dict(what='loop', generator=size, batch=batch, fused_us=tm['fused'], unfused_us=tm['unfused'],
                   uncached_us=tm['uncached'], unfused_over_fused=round(tm['unfused'][0] / tm['fused'][0], 4),
                   uncached_over_cached=round(tm['uncached'][0] / tm['fused'][0], 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del g, versions
        torch.cuda.empty_cache()
    return rows


def repeat_rows(d):
    import lpips
    import stylegan2
    import ppl_cases as pc
    import projection_cases as pj
    from Evaluation.image_projection import project
    percept = lpips.PerceptualLoss(model='net-lin', net='vgg')
    percept.load_state_dict(pc.percept_state_dict(percept.state_dict()))
    percept = percept.to(d).to(memory_format=torch.channels_last)
    rows = []
    for c in pj.TRAJECTORIES:
        if c['kind'] != 'generator':
            continue
        g = stylegan2.Generator(c['size'], pj.LATENT_DIM, 2, channel_multiplier=1)
        g.load_state_dict(synth.state_dict('generator', g.state_dict(), seed=4))
        g = g.to(d).eval().requires_grad_(False)
        runs = []
        for _ in range(2):
            avg_w, noises, target = pj.trajectory_start(c, g, device=d)
            start = [avg_w.clone()] + [n.clone() for n in noises]
            crit = project.ImageReconstructionLoss(device=d, loss='mse+lpips', percept=percept)
            opt = torch.optim.Adam([avg_w] + noises, lr=pj.LR)
            kwargs = {'noise_z': None, 'input_is_latent': True, 'latent_styles': [avg_w], 'noise': noises}
            history = []
            project.optimize(g, kwargs, {'target': target, 'mask': None}, crit, opt, c['iterations'], print_iterations=0,
                             history=history)
            runs.append(([(p.detach() - s).double() for p, s in zip([avg_w] + noises, start)],
                         [float(l) for _, l in history]))
        diffs = [float((p - q).norm() / q.norm()) for p, q in zip(runs[0][0], runs[1][0])]
        loss = max(abs(p - q) / abs(q) for p, q in zip(runs[0][1], runs[1][1]))
        row = dict(what='repeat', case=c['name'], displacement_rel_l2=[float(f'{v:.3e}') for v in diffs],
                   largest=max(diffs), largest_loss_rel=loss)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _t(v):
    return f'{v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})'


def _ms(v):
    return f'{v[0] / 1e3:.2f} ({v[1] / 1e3:.2f} .. {v[2] / 1e3:.2f})'


def markdown(run):
    out = ['# Image projection: the criterion\'s image stage and the projection loop (`tools/bench_projection.py`)', '',
           f"One {run['device']}, fp32.  `{run['command']}`.  HIP events round "
           f"windows of back-to-back calls of at least {run['window']} s; every version warmed up; the versions alternate "
           f"inside each of {run['rounds']} rounds.  Figures: µs (stage) or ms (loop) per call, median round (lowest .. "
           f"highest round).", '',
           '## (a) Stage forward + backward', '',
           '| shape, f | the two kernels alone, µs | TB/s of the bytes they must move (share of 8 TB/s) | '
           '`projection_stage` + autograd, µs | composite + autograd, µs | composite ÷ fused |', '|---|---|---|---|---|---|']
    for r in run['rows']:
        if r['what'] == 'stage':
            out.append(f"| {r['shape']}, {r['f']} | {_t(r['kernel_us'])} | {r['kernel_tbs']} ({r['kernel_of_peak']}) of "
                       f"{r['bytes']} B | {_t(r['fused_us'])} | {_t(r['composite_us'])} | {r['composite_over_fused']} |")
    out += ['', '## (b) One Adam iteration of the projection loop, `mse+lpips`', '',
            '| generator, batch | fused, target features cached, ms | unfused (`FMGAN_NO_PROJECT_FUSE=1`), ms | unfused ÷ '
            'fused | fused, `pre_cache=False`, ms | uncached ÷ cached |', '|---|---|---|---|---|---|']
    for r in run['rows']:
        if r['what'] == 'loop':
            out.append(f"| Generator({r['generator']}), {r['batch']} | {_ms(r['fused_us'])} | {_ms(r['unfused_us'])} | "
                       f"{r['unfused_over_fused']} | {_ms(r['uncached_us'])} | {r['uncached_over_cached']} |")
    out += ['', '## (c) Two runs of the test trajectories in one process', '',
            '| case | relative L2 difference of the displacement: W, then each noise map | largest | largest relative '
            'difference of a step\'s loss |', '|---|---|---|---|']
    for r in run['rows']:
        if r['what'] == 'repeat':
            out.append(f"| {r['case']} | {r['displacement_rel_l2']} | {r['largest']:.3e} | {r['largest_loss_rel']:.3e} |")
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None)
    ap.add_argument('--skip-loops', action='store_true')
    ap.add_argument('--skip-repeat', action='store_true')
    a = ap.parse_args()
    d = torch.device('cuda', 0)
    rows = stage_rows(a, d)
    if not a.skip_loops:
        rows += loop_rows(a, d)
    if not a.skip_repeat:
        rows += repeat_rows(d)
    command = 'python tools/bench_projection.py ' + ' '.join(sys.argv[1:])
    this = dict(device=torch.cuda.get_device_name(0), command=command.strip(), rounds=a.rounds, window=a.window,
                rows=rows)
    for path, text in ((a.json, json.dumps(this, indent=1)), (a.md, markdown(this))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                f.write(text)


if __name__ == '__main__':
    main()
