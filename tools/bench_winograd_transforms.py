#!/usr/bin/env python3
"""Time the Winograd transform kernels of this tree's libfmgan_hip.so against another build of the library, in one process.

    python tools/bench_winograd_transforms.py --other PATH/libfmgan_hip.so [--rounds 5] [--out FILE.md]

Both libraries are loaded side by side through ctypes and called on the same device tensors, alternating, `--rounds` times:
fmgan_wino_input_f32, fmgan_wino_output_f32 (with the StyledConv epilogue: demodulation, per-sample noise, bias, activation)
and fmgan_wino_weight_f32 at the shapes stylegan2.winograd_pays names in the two benchmark workloads (pairs1024: B = 8,
pairs256: B = 32).  Each figure is the mean of a window of back-to-back launches between two device events, after a warm-up.
Beside each kernel a torch copy that moves the same number of bytes (half of them read, half written) is timed in the same
way: the kernel's rate against that copy, and against the 6.29 TB/s copy rate the profiles quote, is what the table states.
Then the outputs of the three steps (V, U, and the whole form's result through torch.bmm) of the two libraries are compared
with torch.equal.  Needs a GPU."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402

COPY_RATE = 6.29e12
# (batch, channels, plane): the plain layers in Winograd form of Generator(1024) at B = 8 and of Generator(256) at B = 32
SHAPES = [(8, 512, 16), (8, 512, 32), (8, 512, 64), (8, 256, 128), (32, 512, 16), (32, 512, 32), (32, 512, 64), (32, 256, 128)]
# whole-form bit comparison: the B = 8 shapes and the shapes of tests/test_winograd_fast.py (b, cin, cout, h, w)
FORM_SHAPES = [(8, 512, 512, 16, 16), (8, 512, 512, 32, 32), (8, 512, 512, 64, 64), (8, 256, 256, 128, 128),
               (2, 8, 8, 8, 16), (1, 4, 12, 6, 24), (2, 3, 5, 4, 6), (1, 5, 7, 8, 16), (3, 4, 4, 6, 24), (2, 2, 3, 4, 40)]


def load(path):
    L = ctypes.CDLL(path)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    for fn, args in ((L.fmgan_wino_weight_f32, [vp, vp, i, i, vp]), (L.fmgan_wino_input_f32, [vp] * 3 + [i] * 4 + [vp]),
                     (L.fmgan_wino_output_f32, [vp] * 6 + [i] * 6 + [f, f, vp])):
        fn.argtypes, fn.restype = args, i
    return L


def timed(fn, bytes_moved):
    """Mean seconds per call of fn() over a window of about 30 ms (at least 10 calls), after three warm-up calls."""
    n = max(10, min(2000, int(0.03 / (bytes_moved / 3e12 + 5e-6))))
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / n


def copy_time(bytes_moved, d):
    src = torch.randn(bytes_moved // 8, device=d)
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), bytes_moved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other', required=True, help='the library to compare against (the parent commit\'s build)')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    d = torch.device('cuda', 0)
    this = os.path.join(ROOT, '3d-fm-gan_amd', 'csrc', 'libfmgan_hip.so')
    libs = {'other': load(a.other), 'this': load(this)}
    stream = torch.cuda.current_stream(d).cuda_stream
    gen = torch.Generator(device=d).manual_seed(5)
    lines = [f'other = {a.other}', f'this = {this}', f'device = {torch.cuda.get_device_name(0)}', '',
             '| kernel | B, C, plane | bytes moved | other: min / max µs | this: min / max µs | copy of the bytes µs | this / copy '
             '| this, TB/s | of 6.29 TB/s | this max < other min |', '|---|---|---|---|---|---|---|---|---|---|']

    def ok(st):
        assert st == 0, st

    def row(kernel, shape, nbytes, calls):
        t = {k: [] for k in libs}
        for _ in range(a.rounds):
            for k in ('other', 'this'):
                t[k].append(timed(calls[k], nbytes))
        tc = copy_time(nbytes, d)
        best = min(t['this'])
        lines.append(f'| {kernel} | {shape} | {nbytes / 1e6:.1f} MB | {min(t["other"]) * 1e6:.1f} / {max(t["other"]) * 1e6:.1f} '
                     f'| {min(t["this"]) * 1e6:.1f} / {max(t["this"]) * 1e6:.1f} | {tc * 1e6:.1f} | {best / tc:.2f} '
                     f'| {nbytes / best / 1e12:.2f} | {nbytes / best / COPY_RATE:.2f} '
                     f'| {"yes" if max(t["this"]) < min(t["other"]) else "NO"} |')
        print(lines[-1], flush=True)

    for (b, c, h) in SHAPES:
        n = b * (h // 2) * (h // 2)
        x = torch.randn(b, c, h, h, device=d, generator=gen)
        s = 1.0 + 0.5 * torch.randn(b, c, device=d, generator=gen)
        v = torch.empty(16, c, n, device=d)
        m = torch.randn(16, c, n, device=d, generator=gen)
        out = torch.empty(b, c, h, h, device=d)
        dm = 0.5 + torch.rand(b, c, device=d, generator=gen)
        noise = torch.randn(b, 1, h, h, device=d, generator=gen)
        nw = torch.tensor([0.3], device=d)
        bias = 0.1 * torch.randn(c, device=d, generator=gen)
        p = lambda t: t.data_ptr()      # noqa: E731
        row('wino_input', (b, c, h), 4 * (x.numel() + v.numel()),
            {k: (lambda L=L: ok(L.fmgan_wino_input_f32(p(x), p(s), p(v), b, c, h, h, stream))) for k, L in libs.items()})
        row('wino_output', (b, c, h), 4 * (m.numel() + out.numel() + noise.numel()),
            {k: (lambda L=L: ok(L.fmgan_wino_output_f32(p(m), p(dm), p(noise), p(nw), p(bias), p(out), b, c, h, h, b, 1, 0.2,
                                                        2 ** 0.5, stream))) for k, L in libs.items()})
        del x, v, m, out
    for c in (512, 256):
        wt = torch.randn(c, 9, c, device=d, generator=gen)
        u = torch.empty(16, c, c, device=d)
        row('wino_weight', (c, c), 4 * (wt.numel() + u.numel()),
            {k: (lambda L=L: ok(L.fmgan_wino_weight_f32(wt.data_ptr(), u.data_ptr(), c, c, stream))) for k, L in libs.items()})

    lines += ['', 'Bits (torch.equal between the two libraries; V, U, and the whole form through torch.bmm with the epilogue):', '']
    differ = 0
    for (b, cin, cout, h, w) in FORM_SHAPES:
        n = b * (h // 2) * (w // 2)
        x = torch.randn(b, cin, h, w, device=d, generator=gen)
        s = 1.0 + 0.5 * torch.randn(b, cin, device=d, generator=gen)
        wt = torch.randn(cin, 9, cout, device=d, generator=gen) / (3 * cin ** 0.5)
        dm = 0.5 + torch.rand(b, cout, device=d, generator=gen)
        noise = torch.randn(b, 1, h, w, device=d, generator=gen)
        nw = torch.tensor([0.3], device=d)
        bias = 0.1 * torch.randn(cout, device=d, generator=gen)
        res = {}
        for k, L in libs.items():
            u = torch.empty(16, cout, cin, device=d)
            v = torch.empty(16, cin, n, device=d)
            out = torch.empty(b, cout, h, w, device=d)
            ok(L.fmgan_wino_weight_f32(wt.data_ptr(), u.data_ptr(), cin, cout, stream))
            ok(L.fmgan_wino_input_f32(x.data_ptr(), s.data_ptr(), v.data_ptr(), b, cin, h, w, stream))
            m = torch.bmm(u, v)
            ok(L.fmgan_wino_output_f32(m.data_ptr(), dm.data_ptr(), noise.data_ptr(), nw.data_ptr(), bias.data_ptr(),
                                       out.data_ptr(), b, cout, h, w, b, 1, 0.2, 2 ** 0.5, stream))
            res[k] = (u, v, out)
        same = [torch.equal(p_, q_) for p_, q_ in zip(res['other'], res['this'])]
        differ += same.count(False)
        lines.append(f'* {(b, cin, cout, h, w)}: U {"equal" if same[0] else "DIFFERS"}, V {"equal" if same[1] else "DIFFERS"}, '
                     f'out {"equal" if same[2] else "DIFFERS"}')
        print(lines[-1], flush=True)
    lines.append(f'\n{differ} of {3 * len(FORM_SHAPES)} tensors differ.')
    print(lines[-1])
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
