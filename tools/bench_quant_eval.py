#!/usr/bin/env python3
"""Quantitative evaluation (Evaluation/quant_eval.py) on the GPU: the fused metric stage against the composite, and the
whole score loops with EVAL_FUSE on against off.

    python tools/bench_quant_eval.py [--rounds R] [--iters N] [--loop-iters M] [--json PATH]

(a) metric stage alone at [64,3,256,256] (the reference's quant_eval_batch_size) and [8,3,1024,1024]:
      kernel     fmgan_face_input_f32 alone, both grey images + L1 partials, outputs preallocated
      fused      op.eval_scores.face_input (kernel + allocation + the sum of the partials)
      composite  op.eval_scores.face_input_composite (Convert_Tensor_For_Face_Recognition_Loss twice + the L1 line)
    Algorithmic bytes: 2 * B * 3 * H * W * 4 read; GB/s and the share of the 8 TB/s HBM peak for the kernel row.
(b) whole loops at 256^2 with Generator(256, 512, 8), one batch per call, the final transfer included:
      Get_Edit_Score   16 photos x 4 renders (the reference's quant_eval_batch_size // 4), randomize_noise=False
      Get_Recon_Score  64 pairs, the real lpips.PerceptualLoss
    EVAL_FUSE = False runs only code that exists without this module's kernel and loop: it is the baseline.
Method: HIP events on the current stream; the versions alternate inside each of R rounds (after a warm-up of each), N
timed calls per version and round; reported: the median over all calls and the lowest / highest round median (spread).
Launches of the library's own kernels are counted through _native.set_observer.
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
from op import _native, eval_scores  # noqa: E402

HBM_PEAK_GBS = 8000.0
STAGE_SHAPES = [(64, 3, 256, 256), (8, 3, 1024, 1024)]


class CountLaunches:
    """Observer that counts the library's launches by name."""
    wants_paths = False

    def __init__(self):
        self.n = {}

    def begin(self, name, info):
        self.n[name] = self.n.get(name, 0) + 1
        return None

    def end(self, token):
        pass


def count(fn):
    obs = CountLaunches()
    _native.set_observer(obs)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _native.set_observer(None)
    return obs.n


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def alternate(versions, rounds, iters, warm=2):
    """{name: (median of all calls, lowest round median, highest round median)} in microseconds."""
    for fn in versions.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_round = {k: [] for k in versions}
    calls = {k: [] for k in versions}
    for _ in range(rounds):
        for name, fn in versions.items():
            ts = []
            for _ in range(iters):
                s.record()
                fn()
                e.record()
                e.synchronize()
                ts.append(s.elapsed_time(e) * 1e3)
            per_round[name].append(median(ts))
            calls[name] += ts
    return {k: (round(median(calls[k]), 2), round(min(per_round[k]), 2), round(max(per_round[k]), 2)) for k in versions}


def stage_rows(a, d):
    L = _native.lib()
    rows = []
    for shape in STAGE_SHAPES:
        b, c, h, w = shape
        x = synth.tensor('bench_qe/a', shape, dist='uniform').to(d)
        y = synth.tensor('bench_qe/b', shape, dist='uniform').to(d)
        k = _native.face_input_pool(w)
        blocks = L.fmgan_face_input_blocks(b, h, w, k)
        ga = torch.empty((b, 1, h // k, w // k), device=d)
        gb = torch.empty_like(ga)
        partial = torch.empty((b, blocks), device=d)
        stream = torch.cuda.current_stream(d).cuda_stream

        def kernel():
            _native.check(L.fmgan_face_input_f32(x.data_ptr(), y.data_ptr(), ga.data_ptr(), gb.data_ptr(),
                                                 partial.data_ptr(), b, h, w, k, stream), 'face_input')

        def fused():
            eval_scores.face_input(x, y, want_gray_b=True, want_l1=True)

        def composite():
            eval_scores.face_input_composite(x, y, want_gray_b=True, want_l1=True)

        f, cmp_ = eval_scores.face_input(x, y, True, True), eval_scores.face_input_composite(x, y, True, True)
        assert torch.equal(f[0], cmp_[0]) and torch.equal(f[1], cmp_[1])
        torch.testing.assert_close(f[2], cmp_[2], rtol=1e-5, atol=0)
        t = alternate(dict(kernel=kernel, fused=fused, composite=composite), a.rounds, a.iters)
        nbytes = 2 * b * 3 * h * w * 4
        gbs = nbytes / (t['kernel'][0] * 1e-6) / 1e9
        row = dict(what='stage', shape=list(shape), k=k, bytes=nbytes, kernel_us=t['kernel'], fused_us=t['fused'],
                   composite_us=t['composite'], kernel_gbs=round(gbs, 1), kernel_of_peak=round(gbs / HBM_PEAK_GBS, 3),
                   fused_over_composite=round(t['composite'][0] / t['fused'][0], 2), launches_fused=count(fused),
                   launches_composite=count(composite))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def _load(module, kind, seed, d):
    module.load_state_dict(synth.state_dict(kind, module.state_dict(), seed=seed))
    return module.to(d).eval().requires_grad_(False)


def loop_rows(a, d):
    import types
    import quant_eval_cases as qc
    import resnet_encoder
    import stylegan2
    import train_3_encoder as T
    from Evaluation import quant_eval as QE
    from psp_encoder_model.encoders import psp_encoders
    e_tsr = _load(resnet_encoder.resnet18(tensor_encoding=True, tensor_transform=False), 'resnet', 5, d)
    e_w = _load(resnet_encoder.resnet18(tensor_encoding=False, tensor_transform=False), 'resnet', 6, d)
    e_wp = _load(psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=14)), 'psp', 7, d)
    g = _load(stylegan2.Generator(256, 512, 8), 'generator', 4, d)
    lpips_model, face_rec_model = T.Module_Fix_Setup(T.default_args(), d)
    models = (e_tsr, e_w, e_wp, g)
    photos16 = synth.tensor('bench_qe/photo16', (16, 3, 256, 256), dist='uniform').to(d)
    renders = [qc.render(f'bench_qe/render{i}', 16, i).to(d) for i in range(4)]
    photos64 = synth.tensor('bench_qe/photo64', (64, 3, 256, 256), dist='uniform').to(d)
    renders64 = qc.render('bench_qe/render64', 64).to(d)
    edit_loader, recon_loader = [[photos16] + renders], [(photos64, renders64)]

    def run(fn, fuse):
        def f():
            prev, QE.EVAL_FUSE = QE.EVAL_FUSE, fuse
            try:
                return fn()
            finally:
                QE.EVAL_FUSE = prev
        return f

    def edit():
        return QE.Get_Edit_Score(edit_loader, d, models, (face_rec_model, None, None), randomize_noise=False)

    def recon():
        return QE.Get_Recon_Score(recon_loader, d, models, (face_rec_model, lpips_model))

    rows = []
    for name, fn, samples in (('Get_Edit_Score 16x4', edit, 64), ('Get_Recon_Score 64', recon, 64)):
        on, off = run(fn, True), run(fn, False)
        t = alternate(dict(fused=on, baseline=off), a.rounds, a.loop_iters, warm=2)
        row = dict(what='loop', name=name, images=samples, fused_us=t['fused'], baseline_us=t['baseline'],
                   baseline_over_fused=round(t['baseline'][0] / t['fused'][0], 3), scores_fused=list(on()),
                   scores_baseline=list(off()), launches_fused=count(on), launches_baseline=count(off))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--loop-iters', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--skip-loops', action='store_true')
    a = ap.parse_args()
    d = torch.device('cuda', 0)
    with torch.no_grad():
        rows = stage_rows(a, d)
        if not a.skip_loops:
            rows += loop_rows(a, d)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, loop_iters=a.loop_iters,
                           rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
