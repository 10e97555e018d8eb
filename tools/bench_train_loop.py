"""The two launches of the training loop against what they replace, on the GPU (profiles/train_loop.md and .json).

  (a) EMA: on the parameter sets of Generator(256) and Generator(1024), EmaPlan.update against `accumulate`, alternated in
      one process in blocks of --block calls, --calls each after warm-up.  Device time per call from events around each
      block; host time per call = the host clock over the block's enqueueing (no synchronisation inside); both include the
      plan's re-validation.  Whether the two leave the same bits is recorded.  The kernel time proper comes from runs of
      their own under the tracer, one size each,
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_loop.py --ema-only --sizes 1024
      and is read back with --kernel-stats 256=DIR 1024=DIR: over 12 * numel bytes it gives TB/s and the share of the 8 TB/s
      HBM peak.
  (b) the loop: bench.py's trainstep256 Trainer (B = 16, LPIPS and ArcFace as load), --iters iterations through train()
      with log_flush 50, against the same iterations in the reference's structure (nine .item() and the line after each
      one), alternated, --reps times; the fused EMA is on in both.  Also the loss_row launch against torch.stack of the same
      nine scalars, host time per call.

    python tools/bench_train_loop.py [--out-dir profiles] [--skip-loop] [--kernel-stats 256=DIR 1024=DIR]
"""
import argparse
import csv
import glob
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_TBS = 8.0


def say(*a):
    print(*a, flush=True)


def generators(size, device):
    import stylegan2
    torch.manual_seed(size)
    G = stylegan2.Generator(size, 512, 8).to(device)
    g_ema = stylegan2.Generator(size, 512, 8).to(device).eval()
    return G, g_ema


def ema_only(sizes, calls, device):
    """For the tracer: `calls` fused updates per size, nothing else of interest."""
    from op.ema import EmaPlan
    for size in sizes:
        G, g_ema = generators(size, device)
        plan = EmaPlan(g_ema, G)
        for _ in range(calls):
            plan.update(0.999)
        torch.cuda.synchronize()
        say(json.dumps({'ema_only': size, 'calls': calls, 'numel': plan._numel, 'blocks': plan._blocks}))


def bench_ema(size, calls, block, device):
    from op.ema import EmaPlan
    from Util.training_util import accumulate
    G, g_ema = generators(size, device)
    decay = 0.5 ** (32 / (10 * 1000))
    plan = EmaPlan(g_ema, G)
    numel, tensors = plan._numel, plan._n
    # same bits?
    import copy
    other = copy.deepcopy(g_ema)
    plan.update(decay)
    accumulate(other, G, decay)
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(g_ema.parameters(), other.parameters()))
    del other
    forms = {'fused': lambda: plan.update(decay), 'accumulate': lambda: accumulate(g_ema, G, decay)}
    for fn in forms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    dev_ms = {k: [] for k in forms}
    host_ms = {k: [] for k in forms}
    for _ in range(max(1, calls // block)):
        for name, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
            t1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            dev_ms[name].append(a.elapsed_time(b) / block)
            host_ms[name].append((t1 - t0) * 1e3 / block)
    rec = {'size': size, 'tensors': tensors, 'numel': numel, 'bytes': 12 * numel, 'blocks': plan._blocks,
           'calls_each': block * max(1, calls // block), 'same_bits': same}
    for name in forms:
        rec[name] = {'device_ms': statistics.median(dev_ms[name]), 'device_ms_min': min(dev_ms[name]),
                     'device_ms_max': max(dev_ms[name]), 'host_ms': statistics.median(host_ms[name]),
                     'host_ms_min': min(host_ms[name]), 'host_ms_max': max(host_ms[name])}
    return rec


def kernel_stats(spec):
    """{size: average ns of train_ema_f32} from rocprofv3's *kernel_stats.csv below each DIR of 'SIZE=DIR'."""
    out = {}
    for item in spec or ():
        size, d = item.split('=', 1)
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                if 'train_ema_f32' in row['Name']:
                    out[int(size)] = {'calls': int(row['Calls']), 'average_ns': float(row['AverageNs'])}
    return out


class Fixed:
    """A loader that hands train_iteration its triple (as dataset.BankLoader does): bench.py's synthetic pairs."""

    def __init__(self, batch, size, device):
        gen = torch.Generator(device='cpu').manual_seed(1234)
        self.photo = (torch.rand(batch, 3, 256, 256, generator=gen) * 2 - 1).to(device)
        self.render = (torch.rand(batch, 3, size, size, generator=gen) * 2 - 1).to(device)
        self.ref = (torch.rand(batch, 3, size, size, generator=gen) * 2 - 1).to(device)

    def training_batch(self, pair=False, even_only=False):
        step = 2 if even_only else 1
        return self.photo[::step], self.render[::step], self.ref[::step]


def reference_structure(T, tr, loaders, iters, log):
    """The same iterations with the reference's Print_Train_Status after each: nine .item() (train_3_encoder.py:641-651)."""
    from op.loss_log import NAMES
    while tr.iter_idx < iters:
        i = tr.iter_idx
        t0 = time.time()
        ld, ds_flag, extreme = tr.train_iteration(*loaders[:3])
        values = {k: ld[k].mean().item() if k in ld else 0.0 for k in NAMES}
        log.write(T.Train_Status_Line(i, time.time() - t0, ds_flag, extreme, values))
        tr.Sample_Eval_Save_Ckpt(None, None, None, None, None, log=log)


def bench_loop(iters, reps, device):
    import tempfile
    import bench
    bench.warm_miopen_cache()
    exp_dir = tempfile.mkdtemp(prefix='bench_train_loop_')
    import train_3_encoder as T
    wl = bench.WORKLOADS['trainstep256']
    nets = bench.build_models(wl['size'], device)
    for m in nets.values():
        m.requires_grad_(True)
    _, tr = bench.make_trainstep(nets, wl['batch'], device, 0, 1, wl['size'], loss_nets=True)
    args = tr.args
    args.ema_fuse, args.log_flush, args.iter, args.device = True, 50, iters, str(device)
    loaders = (Fixed(wl['batch'], wl['size'], device),) * 3 + (None,)

    def restart():
        tr.iter_idx, tr.ds_count = 0, 0

    def ledger_run():
        restart()
        T.train(args, loaders, (None, None), tr, None, exp_dir, io.StringIO())

    def reference_run():
        restart()
        reference_structure(T, tr, loaders, iters, io.StringIO())

    args.iter = 16
    say('loop: warm-up, 16 iterations of each structure')
    tr.iter_idx = 0
    reference_structure(T, tr, loaders, 16, io.StringIO())
    ledger_run()
    args.iter = iters
    torch.cuda.synchronize()
    ms = {'ledger': [], 'item': []}
    for r in range(reps):
        for name, run in (('ledger', ledger_run), ('item', reference_run)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / iters)
            say(f'loop: repeat {r} {name}: {ms[name][-1]:.2f} ms / iteration')
    return {'workload': 'trainstep256, B = 16, LPIPS + ArcFace as load, ema_fuse on in both', 'iterations': iters,
            'log_flush': 50, 'ms_per_iteration': ms,
            'median': {k: statistics.median(v) for k, v in ms.items()},
            'spread': {k: max(v) - min(v) for k, v in ms.items()}}


def bench_row(device, calls=1000, block=100):
    from op import _native
    vals = [torch.full((), 0.5 + i, device=device) for i in range(9)]
    ring = torch.zeros((2, 16), device=device)
    forms = {'loss_row': lambda: _native.loss_row(vals, ring[0]), 'torch.stack': lambda: torch.stack(vals, out=ring[1, :9])}
    for fn in forms.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(calls // block):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
            us[name].append((time.perf_counter() - t0) * 1e6 / block)
            torch.cuda.synchronize()
    assert torch.equal(ring[0, :9], ring[1, :9])
    return {k: {'host_us': statistics.median(v), 'host_us_min': min(v), 'host_us_max': max(v)} for k, v in us.items()}


def report(res):
    lines = ['# The training loop\'s two launches (`tools/bench_train_loop.py`, MI355X)', '',
             '## (a) EMA of a parameter set: `EmaPlan.update` (one launch) against `accumulate` (two aten launches per tensor)', '',
             'Alternated in one process; medians over the blocks (min – max); both include the plan\'s re-validation.', '',
             '| Generator | tensors | elements | fused device ms | accumulate device ms | fused host ms | accumulate host ms | '
             'same bits | kernel µs (tracer) | TB/s | share of 8 TB/s |', '|---|---|---|---|---|---|---|---|---|---|---|']
    for e in res['ema']:
        k = res.get('kernel', {}).get(str(e['size'])) or res.get('kernel', {}).get(e['size'])
        f, c = e['fused'], e['accumulate']
        if k:
            tbs = e['bytes'] / k['average_ns'] / 1e3
            tail = f"{k['average_ns'] / 1e3:.1f} | {tbs:.2f} | {100 * tbs / HBM_PEAK_TBS:.0f} %"
        else:
            tail = 'not measured | not measured | not measured'
        lines.append(f"| {e['size']} | {e['tensors']} | {e['numel']} | {f['device_ms']:.4f} ({f['device_ms_min']:.4f} – "
                     f"{f['device_ms_max']:.4f}) | {c['device_ms']:.4f} ({c['device_ms_min']:.4f} – {c['device_ms_max']:.4f}) | "
                     f"{f['host_ms']:.4f} ({f['host_ms_min']:.4f} – {f['host_ms_max']:.4f}) | {c['host_ms']:.4f} "
                     f"({c['host_ms_min']:.4f} – {c['host_ms_max']:.4f}) | {e['same_bits']} | {tail} |")
    if res.get('loop'):
        lp = res['loop']
        lines += ['', '## (b) `train()` with the ledger against nine `.item()` per iteration', '',
                  f"{lp['workload']}; {lp['iterations']} iterations per run, log_flush {lp['log_flush']}, alternated.", '',
                  '| structure | ms / iteration per repeat | median | spread |', '|---|---|---|---|']
        for k, label in (('ledger', '`train()` + LossLedger'), ('item', 'nine `.item()` after every iteration')):
            lines.append(f"| {label} | {', '.join(f'{v:.2f}' for v in lp['ms_per_iteration'][k])} | {lp['median'][k]:.2f} | "
                         f"{lp['spread'][k]:.2f} |")
    if res.get('row'):
        lines += ['', '## One row of the log: host time per call', '', '| form | µs (min – max) |', '|---|---|']
        for k, v in res['row'].items():
            lines.append(f"| `{k}` | {v['host_us']:.1f} ({v['host_us_min']:.1f} – {v['host_us_max']:.1f}) |")
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--block', type=int, default=50)
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ema-only', action='store_true')
    ap.add_argument('--skip-loop', action='store_true')
    ap.add_argument('--kernel-stats', nargs='*')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_train_loop.py needs a GPU'
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    if a.ema_only:
        return ema_only(a.sizes, a.calls, device)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {'device': torch.cuda.get_device_name(0), 'ema': [], 'kernel': kernel_stats(a.kernel_stats)}
    for size in a.sizes:
        res['ema'].append(bench_ema(size, a.calls, a.block, device))
        say(json.dumps(res['ema'][-1]))
    res['row'] = bench_row(device)
    say(json.dumps(res['row']))
    if not a.skip_loop:
        res['loop'] = bench_loop(a.iters, a.reps, device)
    with open(os.path.join(a.out_dir, 'train_loop.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    with open(os.path.join(a.out_dir, 'train_loop.md'), 'w') as f:
        f.write(report(res))
    say(report(res))


if __name__ == '__main__':
    main()
