"""Fused against composite FullBatchLBFGS on the GPU, alternating in one process (profiles/lbfgs.md).

  (a) the optimiser alone: a cheap quadratic closure over tensors of the shapes Image_Projector optimises for
      Generator(256) and Generator(1024) in W+ with noise maps, B = 1, history_size 10;
  (b) Image_Projector's loop (project.optimize) on Generator(256): time per step with and without the closure.

Times: wall time per step between synchronisations, and the time between HIP events around every op/_native bracket.
Prints one JSON line per measurement and a summary; --out writes them to a file as well.

    python tools/bench_lbfgs.py [--steps 12] [--reps 3] [--sizes 256 1024] [--skip-projector] [--out FILE]

Kernel times proper come from a run of its own under the tracer, one size at a time:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_lbfgs.py --sizes 1024 --reps 1 --skip-projector
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from Evaluation.image_projection import LBFGS, project  # noqa: E402
from op import _native  # noqa: E402


class EventObserver:
    """HIP events around every bracket; totals() synchronises and returns {name: (launches, milliseconds)}."""
    wants_paths = False

    def __init__(self):
        self.spans = []

    def begin(self, name, info):
        start = torch.cuda.Event(enable_timing=True)
        start.record()
        return name, start

    def end(self, token):
        name, start = token
        stop = torch.cuda.Event(enable_timing=True)
        stop.record()
        self.spans.append((name, start, stop))

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.spans:
            n, ms = out.get(name, (0, 0.0))
            out[name] = (n + 1, ms + a.elapsed_time(b))
        self.spans = []
        return out


def projector_shapes(size, batch=1, style_dim=512):
    """Shapes of [avg_W] + noises as Image_Projector builds them for Generator(size) in W+."""
    log = size.bit_length() - 1
    shapes = [(batch, 2 * log - 2, style_dim), (1, 1, 4, 4)]
    for i in range(3, log + 1):
        shapes += [(1, 1, 2 ** i, 2 ** i)] * 2
    return shapes


class Quadratic(torch.autograd.Function):
    """0.5 sum a x^2 over one flat buffer the parameters are views of: three launches forward, one backward."""

    @staticmethod
    def forward(ctx, flat, a, *params):
        ctx.flat, ctx.a, ctx.shapes = flat, a, [p.shape for p in params]
        return 0.5 * (a * flat * flat).sum()

    @staticmethod
    def backward(ctx, grad):
        g = (ctx.a * ctx.flat) * grad
        out, off = [], 0
        for s in ctx.shapes:
            n = s.numel()
            out.append(g[off:off + n].view(s))
            off += n
        return (None, None) + tuple(out)


def optimiser_alone(size, fuse, steps, dev):
    LBFGS.FUSE = fuse
    shapes = projector_shapes(size)
    n = sum(torch.Size(s).numel() for s in shapes)
    gen = torch.Generator().manual_seed(size)
    flat = torch.randn(n, generator=gen).to(dev)
    a = (1 + 2 * torch.rand(n, generator=gen)).to(dev)
    params, off = [], 0
    for s in shapes:
        k = torch.Size(s).numel()
        params.append(flat[off:off + k].view(s).requires_grad_(True))
        off += k
    opt = LBFGS.FullBatchLBFGS(params, lr=1, history_size=10)

    def closure():
        opt.zero_grad()
        return Quadratic.apply(flat, a, *params)

    loss = closure()
    loss.backward()
    obs = EventObserver()
    walls, ls = [], []
    for j in range(steps):
        if j == 2:      # two steps of warm-up; the history fills over the timed ones
            _native.set_observer(obs if fuse else None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, _, t, ls_step, _, _, _, fail = opt.step({'closure': closure, 'current_loss': loss, 'max_ls': 10})
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        ls.append(int(ls_step))
    _native.set_observer(None)
    assert (opt._fused is not None) == fuse
    timed = walls[2:]
    return {'what': 'optimiser_alone', 'size': size, 'n': n, 'fused': fuse, 'steps_timed': len(timed),
            'wall_ms_min': min(timed), 'wall_ms_mean': sum(timed) / len(timed), 'wall_ms_max': max(timed),
            'ls_steps': ls, 'loss': float(loss), 'history': len(opt.state['global_state']['old_dirs']),
            'brackets': {k: {'launches': c, 'ms': ms} for k, (c, ms) in obs.totals().items()}}


def projector_loop(fuse, steps, dev, size=256):
    import stylegan2
    from Evaluation.image_projection import image_projector as IP
    LBFGS.FUSE = fuse
    torch.manual_seed(1)
    g = stylegan2.Generator(size, 512, 8).to(dev).eval().requires_grad_(False)
    with torch.no_grad():
        target = g([torch.randn(1, 512, device=dev)]).clamp(-1, 1)
    avg_w = IP.Get_Avg_W_as_Latent(g, dev, True).clone().requires_grad_(True)
    noises = [n.requires_grad_(True) for n in g.make_noise()]
    kwargs = {'noise_z': None, 'input_is_latent': True, 'latent_styles': [avg_w], 'noise': noises}
    crit = project.ImageReconstructionLoss(device=dev, loss='mse+lpips')
    opt = LBFGS.FullBatchLBFGS([avg_w] + noises, lr=1)
    closure_ms = [0.0]

    # the closure is the model and the criterion: the model call is timed between synchronisations
    def model(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = g(**kw)
        torch.cuda.synchronize()
        closure_ms[0] += (time.perf_counter() - t0) * 1e3
        return out

    history = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    project.optimize(model, kwargs, {'target': target, 'mask': None}, crit, opt, steps - 1, print_iterations=0,
                     history=history)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    assert (opt._fused is not None) == fuse
    return {'what': 'projector_loop', 'size': size, 'fused': fuse, 'steps': steps, 'wall_ms_per_step': wall / steps,
            'generator_forward_ms_per_step': closure_ms[0] / steps,
            'without_generator_forward_ms_per_step': (wall - closure_ms[0]) / steps,
            'loss_first': float(history[0][1]), 'loss_last': float(history[-1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--skip-projector', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    rows = []
    for size in args.sizes:
        for rep in range(args.reps):
            for fuse in (True, False):
                rows.append(dict(optimiser_alone(size, fuse, args.steps, dev), rep=rep))
                print(json.dumps(rows[-1]), flush=True)
    if not args.skip_projector:
        for fuse in (True, False):      # warm-up, not recorded: MIOpen's find and the allocator's first blocks
            projector_loop(fuse, 3, dev)
        for rep in range(args.reps):
            for fuse in (True, False):
                rows.append(dict(projector_loop(fuse, 10, dev), rep=rep))
                print(json.dumps(rows[-1]), flush=True)
    summary = {}
    for size in args.sizes:
        f = [r['wall_ms_mean'] for r in rows if r['what'] == 'optimiser_alone' and r['size'] == size and r['fused']]
        c = [r['wall_ms_mean'] for r in rows if r['what'] == 'optimiser_alone' and r['size'] == size and not r['fused']]
        summary[f'optimiser_alone_{size}'] = {'slowest_fused_ms': max(f), 'fastest_composite_ms': min(c),
                                              'ordering_holds': max(f) < min(c)}
    p = [r for r in rows if r['what'] == 'projector_loop']
    if p:
        f = [r['wall_ms_per_step'] for r in p if r['fused']]
        c = [r['wall_ms_per_step'] for r in p if not r['fused']]
        summary['projector_loop_256'] = {'fused_ms_per_step': f, 'composite_ms_per_step': c,
                                         'no_slower': min(f) <= max(c)}
    print(json.dumps({'summary': summary}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump({'rows': rows, 'summary': summary}, fh, indent=1)


if __name__ == '__main__':
    main()
