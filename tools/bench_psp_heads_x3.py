"""Per-layer A/B of the pSp style heads' first convolution: conv3x3s2_bf16x3 (split-operand bf16 contraction, fp32
accumulation) against MIOpen's fp32 convolution + fused_bias_act, alternating in one process; then a whole
GradualStyleBlock with the switch on (kernel output channels_last / NCHW) and off.  Prints one JSON line per measurement
(profiles/psp_heads_x3.md).

    python tools/bench_psp_heads_x3.py [--batch 8] [--rounds 5] [--reps 10]
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
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    from op import _native, fused_leaky_relu
    from psp_encoder_model.encoders import psp_encoders
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(1)
    B = args.batch
    with torch.no_grad():
        for hw in (64, 32):
            x = torch.randn(B, 512, hw, hw, generator=g)
            w = torch.randn(512, 512, 3, 3, generator=g) * (2.0 / 4608) ** 0.5
            bias = torch.randn(512, generator=g) * 0.1
            xd, wd, bd = x.to(dev), w.to(dev).contiguous(memory_format=torch.channels_last), bias.to(dev)
            xcl = xd.contiguous(memory_format=torch.channels_last)
            img = _native.conv_weight_to_bf16x3(wd)

            def hip():
                return _native.conv3x3s2_bf16x3(xd, img, bd, 512, 0.01)

            def hip_nhwc_out():
                return _native.conv3x3s2_bf16x3(xd, img, bd, 512, 0.01, channels_last=True)

            def miopen():
                y = F.conv2d(xcl, wd, None, 2, 1)
                n, c, h, ww = y.shape
                return fused_leaky_relu(y.permute(0, 2, 3, 1).reshape(-1, c), bd, 0.01, 1.0).view(n, h, ww, c).permute(0, 3, 1, 2)

            def miopen_conv_only():
                return F.conv2d(xcl, wd, None, 2, 1)

            for f in (hip, hip_nhwc_out, miopen, miopen_conv_only):
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            t = {'hip': [], 'hip_nhwc_out': [], 'miopen': [], 'miopen_conv_only': []}
            for _ in range(args.rounds):
                for name, f in (('hip', hip), ('hip_nhwc_out', hip_nhwc_out), ('miopen', miopen), ('miopen_conv_only', miopen_conv_only)):
                    t[name].append(timed(f, args.reps))
            flop = 2.0 * B * 512 * 512 * 9 * (hw // 2) ** 2
            r64 = F.leaky_relu(F.conv2d(x[:1].double(), w.double(), bias.double(), 2, 1), 0.01)
            m = float(r64.abs().max())
            e_hip = float((_native.conv3x3s2_bf16x3(xd[:1].contiguous(), img, bd, 512, 0.01).cpu().double() - r64).abs().max()) / m
            e_mio = float((F.leaky_relu(F.conv2d(xcl[:1], wd, bd, 2, 1), 0.01).cpu().double() - r64).abs().max()) / m
            out = {'layer': f'{hw}^2->{hw // 2}^2 512->512 B={B}', 'gflop': flop / 1e9}
            for name, v in t.items():
                out[name + '_us'] = [round(u, 1) for u in v]
                out[name + '_tflops_best'] = round(flop / min(v) / 1e6, 1)
            out['err_vs_fp64_hip'] = e_hip
            out['err_vs_fp64_miopen'] = e_mio
            print(json.dumps(out), flush=True)

        # the whole head at 64^2: switch on (tail channels_last / NCHW) and off; input channels_last as in the encoder
        blk = psp_encoders.GradualStyleBlock(512, 512, 64).to(dev)
        feat = torch.randn(B, 512, 64, 64, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        nchw = feat.contiguous()
        for m_ in blk.modules():
            if isinstance(m_, torch.nn.Conv2d):
                m_.weight.data = m_.weight.data.contiguous(memory_format=torch.channels_last)
        modes = {'x3_out_channels_last': (True, True), 'x3_out_nchw': (True, False), 'miopen': (False, True)}
        res = {k: [] for k in modes}

        def run(on, cl):
            psp_encoders.HEADS_X3, psp_encoders.X3_TAIL_CHANNELS_LAST = on, cl
            return blk(feat, nchw if on else None)

        for on, cl in modes.values():
            for _ in range(3):
                run(on, cl)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, (on, cl) in modes.items():
                res[k].append(round(timed(lambda: run(on, cl), args.reps), 1))
        psp_encoders.HEADS_X3, psp_encoders.X3_TAIL_CHANNELS_LAST = True, True
        print(json.dumps({'block': f'GradualStyleBlock(512,512,64) B={B} us per forward', **res}), flush=True)


if __name__ == '__main__':
    main()
