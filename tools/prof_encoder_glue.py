#!/usr/bin/env python3
"""The pSp encoder alone (bench.py's e_wp: IR-SE-18, 18 heads, 256^2 input) under a kernel trace, and the glue table of
profiles/encoder_glue.md.

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/prof_encoder_glue.py run [BATCH]
      eight forwards, each synchronised and followed by a 60 ms pause, so the trace splits into forwards by its gaps;
      FMGAN_NO_ENCODER_FUSE=1 (or the parent commit's tree) gives the module path.
  python tools/prof_encoder_glue.py table BEFORE_kernel_trace.csv AFTER_kernel_trace.csv [BATCH]
      one steady-state forward of each trace (the last but one): wall time, and every kernel whose launch count differs
      between the two or that belongs to csrc/encoder_glue.hip, side by side — that is the glue, nothing is hand-picked.
      For the glue kernels also each launch with its time and the GB/s of the tensors it has to move.
  python tools/prof_encoder_glue.py time [BATCH]
      no tracer: input layer + body, and the whole encoder, module path and fused path alternating in one process —
      host time to enqueue a forward and time until the GPU has finished it (minimum / median of 10).
"""
import csv
import os
import re
import sys
import time
import types
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(batch):
    sys.path[:0] = [ROOT, os.path.join(ROOT, '3d-fm-gan_amd')]
    import torch
    from psp_encoder_model.encoders import psp_encoders
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(0)
    opts = types.SimpleNamespace(input_nc=3, n_styles=18)
    enc = psp_encoders.GradualStyleEncoder(18, 'ir_se', opts).eval().requires_grad_(False).cuda()
    x = torch.randn(batch, 3, 256, 256, device='cuda')
    with torch.no_grad():
        for _ in range(8):
            enc(x)
            torch.cuda.synchronize()
            time.sleep(0.06)


def timed(batch):
    sys.path[:0] = [ROOT, os.path.join(ROOT, '3d-fm-gan_amd')]
    import torch
    from psp_encoder_model.encoders import psp_encoders, helpers
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(0)
    opts = types.SimpleNamespace(input_nc=3, n_styles=18)
    enc = psp_encoders.GradualStyleEncoder(18, 'ir_se', opts).eval().requires_grad_(False).cuda()
    x = torch.randn(batch, 3, 256, 256, device='cuda').contiguous(memory_format=torch.channels_last)
    enc._to_channels_last()

    def body():
        if helpers.fused_body(enc.input_layer, enc.body, x) is None:
            enc.body(enc.input_layer(x))

    with torch.no_grad():
        for what, fn in (('input layer + body', body), ('whole encoder', lambda: enc.forward_deferred(x))):
            for fuse in (False, True, False, True):
                helpers.ENCODER_FUSE = fuse
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                host, done = [], []
                for _ in range(10):
                    t0 = time.perf_counter()
                    fn()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    host.append((t1 - t0) * 1e3)
                    done.append((time.perf_counter() - t0) * 1e3)
                print(f"{what}, {'fused' if fuse else 'modules'}: enqueue {min(host):.3f} / {sorted(host)[5]:.3f} ms, "
                      f'finished {min(done):.3f} / {sorted(done)[5]:.3f} ms', flush=True)


def steady_forward(path, gap_ns=30_000_000):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    segs, cur = [], [rows[0]]
    for a, b in zip(rows, rows[1:]):
        if int(b['Start_Timestamp']) - int(a['End_Timestamp']) > gap_ns:
            segs.append(cur)
            cur = []
        cur.append(b)
    segs.append(cur)
    return [s for s in segs if len(s) > 50][-2]


def short(name, n=72):
    name = re.sub(r'\(anonymous namespace\)::', '', name)
    name = re.sub(r'^void ', '', name)
    return name if len(name) <= n else name[:n - 3] + '...'


def dur(r):
    return int(r['End_Timestamp']) - int(r['Start_Timestamp'])


def glue_bytes(batch):
    """Bytes each glue launch of one IR-SE-18 forward has to move (fp32), in launch order per kernel."""
    mb = lambda c, hw: 4.0 * batch * c * hw * hw
    units = [(64, 128, False), (64, 128, False), (128, 64, True), (128, 64, False), (256, 32, True), (256, 32, False),
             (512, 16, True), (512, 16, False)]                     # (depth, output size, convolution shortcut)
    out = {'eg_bn_prelu': [mb(64, 256) * 2 + mb(64, 128)], 'eg_se_pool': [], 'eg_ir_tail': []}
    for i, (c, hw, conv) in enumerate(units):
        out['eg_se_pool'].append(mb(c, hw))
        # r + shortcut in, out + out_next (all but the last unit)
        out['eg_ir_tail'].append(mb(c, hw) * (3 + (i + 1 < len(units))))
    return out


def table(before, after, batch):
    segs = {'before': steady_forward(before), 'after': steady_forward(after)}
    agg = {k: defaultdict(lambda: [0, 0]) for k in segs}
    for k, seg in segs.items():
        wall = (max(int(r['End_Timestamp']) for r in seg) - int(seg[0]['Start_Timestamp'])) / 1e6
        print(f'{k}: one forward = {len(seg)} kernels, wall {wall:.3f} ms, sum of kernel time '
              f'{sum(dur(r) for r in seg) / 1e6:.3f} ms\n')
        for r in seg:
            a = agg[k][short(r['Kernel_Name'])]
            a[0] += 1
            a[1] += dur(r)
    names = sorted(set(agg['before']) | set(agg['after']),
                   key=lambda n: -(agg['before'][n][1] + agg['after'][n][1]))
    # MIOpen's convolution kernels and their helpers: a launch count that differs there is the SE module's 1x1 convolutions
    # (now inside se_gate) or the per-process solver search choosing another kernel for a layer
    conv = re.compile(r'igemm|grouped_conv|naive_conv|Conv|SubTensorOp|fillBuffer|Cijk')
    for title, want_conv in (('non-convolution kernels', False), ('convolution kernels and their helpers', True)):
        print(f'{title}:\n')
        print('| kernel | launches before | us before | launches after | us after |')
        print('|---|---|---|---|---|')
        tot = [0, 0, 0, 0]
        for n in names:
            b, a = agg['before'][n], agg['after'][n]
            if (b[0] == a[0] and not n.startswith('eg_')) or bool(conv.search(n)) != want_conv:
                continue
            print(f'| `{n}` | {b[0]} | {b[1] / 1e3:.1f} | {a[0]} | {a[1] / 1e3:.1f} |')
            tot = [tot[0] + b[0], tot[1] + b[1], tot[2] + a[0], tot[3] + a[1]]
        print(f'| **sum** | {tot[0]} | {tot[1] / 1e3:.1f} | {tot[2]} | {tot[3] / 1e3:.1f} |\n')
    need = glue_bytes(batch)
    seen = defaultdict(int)
    print('| glue launch | grid | us | MB moved | GB/s |')
    print('|---|---|---|---|---|')
    for r in segs['after']:
        m = re.search(r'eg_\w+?(?=_f32)', r['Kernel_Name'])
        if not m:
            continue
        k, i = m.group(0), seen[m.group(0)]
        seen[k] += 1
        grid = f"{r['Grid_Size_X']}x{r.get('Grid_Size_Y', '1')}"
        if k in need and i < len(need[k]):
            print(f'| `{k}` #{i} | {grid} | {dur(r) / 1e3:.1f} | {need[k][i] / 1e6:.1f} | {need[k][i] / dur(r):.0f} |')
        else:
            print(f'| `{k}` #{i} | {grid} | {dur(r) / 1e3:.1f} | | |')


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == 'run':
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    elif len(sys.argv) >= 2 and sys.argv[1] == 'time':
        timed(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    elif len(sys.argv) >= 4 and sys.argv[1] == 'table':
        table(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 8)
    else:
        sys.exit(__doc__)
