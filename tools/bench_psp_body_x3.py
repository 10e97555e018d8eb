"""Per-layer A/B of the pSp encoder body's sixteen 3x3 convolutions (IR-SE-18 at a 256^2 photo): conv3x3_bf16x3 (the
split-operand bf16 contraction, fp32 accumulation, with the epilogue the body uses: PReLU for a unit's conv1, none for its
conv2) against MIOpen's fp32 convolution under its measured find (+ aten PReLU where the epilogue replaces it).  Both
sides read and write channels_last tensors and alternate in one process.  Then the style heads' first convolution with an
NCHW against a channels_last input.  One JSON line per measurement (profiles/psp_body_x3.md).

    python tools/bench_psp_body_x3.py [--batch 8] [--rounds 5] [--reps 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '3d-fm-gan_amd')]

import torch
import torch.nn.functional as F

torch.backends.cudnn.benchmark = True

# (name, cin, cout, input size, stride, epilogue) of the body's convolutions, in order
LAYERS = [('u0 conv1', 64, 64, 256, 1, 'prelu'), ('u0 conv2', 64, 64, 256, 2, None),
          ('u1 conv1', 64, 64, 128, 1, 'prelu'), ('u1 conv2', 64, 64, 128, 1, None),
          ('u2 conv1', 64, 128, 128, 1, 'prelu'), ('u2 conv2', 128, 128, 128, 2, None),
          ('u3 conv1', 128, 128, 64, 1, 'prelu'), ('u3 conv2', 128, 128, 64, 1, None),
          ('u4 conv1', 128, 256, 64, 1, 'prelu'), ('u4 conv2', 256, 256, 64, 2, None),
          ('u5 conv1', 256, 256, 32, 1, 'prelu'), ('u5 conv2', 256, 256, 32, 1, None),
          ('u6 conv1', 256, 512, 32, 1, 'prelu'), ('u6 conv2', 512, 512, 32, 2, None),
          ('u7 conv1', 512, 512, 16, 1, 'prelu'), ('u7 conv2', 512, 512, 16, 1, None)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us


def alternate(fns, rounds, reps):
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(round(timed(f, reps), 1))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    from op import _native
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(1)
    B = args.batch
    with torch.no_grad():
        for name, cin, cout, hw, stride, epi in LAYERS:
            x = torch.randn(B, cin, hw, hw, generator=g)
            w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
            slope = torch.randn(cout, generator=g) * 0.25
            xcl = x.to(dev).contiguous(memory_format=torch.channels_last)
            wd, sd = w.to(dev).contiguous(memory_format=torch.channels_last), slope.to(dev)
            img = _native.conv_weight_to_bf16x3(wd)

            def hip():
                return _native.conv3x3_bf16x3(xcl, img, cout, stride, epi, sd if epi else None, channels_last=True)

            def miopen():
                y = F.conv2d(xcl, wd, None, stride, 1)
                return F.prelu(y, sd) if epi else y

            t = alternate({'hip': hip, 'miopen': miopen}, args.rounds, args.reps)
            oh = (hw - 1) // stride + 1
            flop = 2.0 * B * cin * cout * 9 * oh * oh
            r64 = F.conv2d(x[:1].double(), w.double(), None, stride, 1)
            if epi:
                r64 = F.prelu(r64, slope.double())
            m = float(r64.abs().max())
            a = _native.conv3x3_bf16x3(xcl[:1], img, cout, stride, epi, sd if epi else None, channels_last=True)
            y = F.conv2d(xcl[:1], wd, None, stride, 1)
            y = F.prelu(y, sd) if epi else y
            out = {'layer': f'{name} {cin}->{cout} {hw}^2 s{stride} B={B}', 'epilogue': epi or 'none', 'gflop': round(flop / 1e9, 2)}
            for k, v in t.items():
                out[k + '_us'] = v
                out[k + '_tflops_best'] = round(flop / min(v) / 1e6, 1)
            out['served_by_rule'] = max(t['hip']) < min(t['miopen'])       # the kernel's slowest round beats MIOpen's fastest
            out['err_vs_fp64_hip'] = float((a.cpu().double() - r64).abs().max()) / m
            out['err_vs_fp64_miopen'] = float((y.cpu().double() - r64).abs().max()) / m
            print(json.dumps(out), flush=True)

        # the heads' first convolution (512 -> 512, 64^2 -> 32^2, bias + LeakyReLU): NCHW against channels_last input
        x = torch.randn(B, 512, 64, 64, generator=g).to(dev)
        xcl = x.contiguous(memory_format=torch.channels_last)
        wd = (torch.randn(512, 512, 3, 3, generator=g) * (2.0 / 4608) ** 0.5).to(dev)
        bd = (torch.randn(512, generator=g) * 0.1).to(dev)
        img = _native.conv_weight_to_bf16x3(wd)
        fns = {'nchw_in': lambda: _native.conv3x3s2_bf16x3(x, img, bd, 512, 0.01, channels_last=True),
               'channels_last_in': lambda: _native.conv3x3s2_bf16x3(xcl, img, bd, 512, 0.01, channels_last=True),
               'nchw_copy': lambda: xcl.contiguous()}
        same = torch.equal(fns['nchw_in'](), fns['channels_last_in']())
        t = alternate(fns, args.rounds, args.reps)
        print(json.dumps({'layer': f'head conv0 512->512 64^2 s2 B={B} us', **t, 'same_bits': same}), flush=True)


if __name__ == '__main__':
    main()
