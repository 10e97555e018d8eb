"""Per-layer A/B of the pSp style heads' 16- and 8-wide stride-2 convolutions: conv3x3_tail_bf16x3 (the narrow-tile
members of the split-operand family, bias + LeakyReLU in the epilogue) against MIOpen's fp32 convolution under its
measured find + fused_bias_act, both channels_last in and out, alternating in one process; and, for the tile it
replaces on these shapes, the family's 32-column kernel.  Prints one JSON line per layer (profiles/psp_tail_x3.md).

    python tools/bench_psp_tail_x3.py [--batch 8 32] [--rounds 5] [--reps 10]

FMGAN_LIB=<another build of csrc> measures a different tile of TailTile (csrc/conv3x3_x3.hip).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, '3d-fm-gan_amd')]

import torch
import torch.nn.functional as F


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    from op import _native, fused_leaky_relu
    torch.backends.cudnn.benchmark = True          # MIOpen's measured find, as the encoder runs it in bench.py
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for B in args.batch:
            for hw in (32, 16):
                x = torch.randn(B, 512, hw, hw, generator=g)
                w = torch.randn(512, 512, 3, 3, generator=g) * (2.0 / 4608) ** 0.5
                bias = torch.randn(512, generator=g) * 0.1
                wd, bd = w.to(dev).contiguous(memory_format=torch.channels_last), bias.to(dev)
                xcl = x.to(dev).contiguous(memory_format=torch.channels_last)
                img = _native.conv_weight_to_bf16x3(wd)

                def tail():
                    return _native.conv3x3_tail_bf16x3(xcl, img, bd, 512, 0.01)

                def wide_tile():
                    return _native.conv3x3_bf16x3(xcl, img, 512, 2, 'lrelu', bd, 0.01, channels_last=True)

                def miopen():
                    y = F.conv2d(xcl, wd, None, 2, 1)
                    n, c, h, ww = y.shape
                    return fused_leaky_relu(y.permute(0, 2, 3, 1).reshape(-1, c), bd, 0.01, 1.0).view(n, h, ww, c).permute(0, 3, 1, 2)

                def miopen_conv_only():
                    return F.conv2d(xcl, wd, None, 2, 1)

                fns = (('tail', tail), ('wide_tile', wide_tile), ('miopen', miopen), ('miopen_conv_only', miopen_conv_only))
                for _, f in fns:
                    for _ in range(3):
                        f()
                torch.cuda.synchronize()
                t = {name: [] for name, _ in fns}
                for _ in range(args.rounds):
                    for name, f in fns:
                        t[name].append(timed(f, args.reps))
                flop = 2.0 * B * 512 * 512 * 9 * (hw // 2) ** 2
                r64 = F.leaky_relu(F.conv2d(x[:1].double(), w.double(), bias.double(), 2, 1), 0.01)
                m = float(r64.abs().max())
                e_hip = float((_native.conv3x3_tail_bf16x3(xcl[:1], img, bd, 512, 0.01).cpu().double() - r64).abs().max()) / m
                e_mio = float((miopen()[:1].cpu().double() - r64).abs().max()) / m
                out = {'layer': f'{hw}^2->{hw // 2}^2 512->512 B={B}', 'gflop': round(flop / 1e9, 2),
                       'tile': _native.conv3x3_tail_bf16x3_select(B, 512, 512, hw, hw)}
                for name, v in t.items():
                    out[name + '_us'] = [round(u, 1) for u in v]
                    out[name + '_tflops_best'] = round(flop / min(v) / 1e6, 1)
                out['rule_tail_slowest_beats_miopen_fastest'] = max(t['tail']) < min(t['miopen'])
                out['err_vs_fp64_tail'] = e_hip
                out['err_vs_fp64_miopen'] = e_mio
                print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
