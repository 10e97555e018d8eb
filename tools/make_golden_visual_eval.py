#!/usr/bin/env python3
"""Generate tests/golden/visual_eval.npz and visual_eval.json by the reference's Evaluation/visual_eval.py on CPU.

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_visual_eval.py
The reference is imported exactly as tools/make_golden.py imports it (JIT and torchvision stubbed; importing that module
does it), its visual_eval module with `imageio` stubbed.  With the full-width seeded networks of
tools/make_golden_reanimate.py, built once per dtype, it runs the reference's own Get_Batch_Eval_Result (two sets of
VAL_SET_LEN images) and Get_Multi_Photo_Multi_Render_Result (three photo / render frame pairs; its GIF loader replaced by
the synthetic frames), in fp32 and in float64; the float outputs are taken from the reference's own forward by wrapping
the name the module calls.  Inputs and weights come from tests/synth.py on both sides; the files hold OUTPUTS only:
strided samples of the float outputs (`/sub`, `/sub64`), their statistics (`/stats`) and the strided uint8 images (`/u8`),
and, as JSON, the host selections of the pickers, the path helpers and the test drivers on fabricated directories, and
the key list of the reference's checkpoint.  Before writing, the reference's fp32 uint8 images are held against its own
float64 run by the rule the tests apply (tests/visual_eval_cases.py::u8_rule_violations)."""
import json
import os
import re
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (stubs the JIT, puts the reference and tests/ on sys.path)
import visual_eval_cases as vc  # noqa: E402

sys.modules.setdefault('imageio', types.ModuleType('imageio'))
import Evaluation.visual_eval as ref_ve  # noqa: E402


def networks(c, dt):
    n_latent = int(np.log2(c['size'])) * 2 - 2
    e_tsr, e_w, e_wp = mg.build_encoders(n_latent)
    g = mg.stylegan2.Generator(c['size'], 512, 8)
    g.load_state_dict(mg.synth.state_dict('generator', g.state_dict(), seed=4))
    g.eval()
    for m in (e_tsr, e_w, e_wp, g):
        m.to(dt)
    return e_tsr, e_w, e_wp, mg._GWrap(g)


class Recorded:
    """Stands in for the forward the reference's module calls: the same call, its float output kept."""

    def __init__(self):
        self.real = ref_ve.Forward_Inference_3_Encoder
        self.outputs = []

    def __call__(self, *a, **kw):
        out = self.real(*a, **kw)
        self.outputs.append(out.detach().clone())
        return out

    def __enter__(self):
        ref_ve.Forward_Inference_3_Encoder = self
        return self

    def __exit__(self, *exc):
        ref_ve.Forward_Inference_3_Encoder = self.real
        return False


def run_batch(dt, modules):
    c = vc.BATCH
    imgs = [t.to(dt) for t in vc.batch_inputs(c)]
    with Recorded() as rec:
        u8 = ref_ve.Get_Batch_Eval_Result(imgs, modules, **vc.fwd_kwargs(c))
    return np.stack(u8), torch.cat(rec.outputs, 0)


def run_video(dt, modules):
    c = vc.VIDEO
    p, r = vc.video_inputs(c)
    frames = {'photo.gif': [t.to(dt) for t in p], 'render.gif': [t.to(dt) for t in r]}
    loader = ref_ve.Load_GIF_As_Img_List
    ref_ve.Load_GIF_As_Img_List = lambda path, transform: frames[path]
    try:
        with Recorded() as rec:
            u8 = ref_ve.Get_Multi_Photo_Multi_Render_Result('photo.gif', 'render.gif', modules, None, 'cpu',
                                                            **vc.fwd_kwargs(c))
    finally:
        ref_ve.Load_GIF_As_Img_List = loader
    return np.stack(u8), torch.cat(rec.outputs, 0)


def images():
    out = {}
    with torch.no_grad():
        runs = {}
        for dt in (torch.float32, torch.float64):
            modules = networks(vc.BATCH, dt)
            runs[dt] = {'batch': run_batch(dt, modules), 'video': run_video(dt, modules)}
            print(' ', dt, 'done', flush=True)
    for key, c in (('batch', vc.BATCH), ('video', vc.VIDEO)):
        s = c['stride']
        u8, img = runs[torch.float32][key]
        u8_64, img64 = runs[torch.float64][key]
        n = c['name']
        out[n + '/sub'] = mg.subsample(img, s)
        out[n + '/stats'] = mg.stats(img)
        out[n + '/sub64'] = mg.subsample(img64, s)
        out[n + '/u8'] = u8[:, ::s, ::s].copy()
        # the output images inside the uint8 list: every second one after each photo (batch), all of them (video)
        where = [i for i in range(len(u8)) if i % 5 in (2, 4)] if key == 'batch' else list(range(len(u8)))
        bad = vc.u8_rule_violations(u8[where], u8_64[where], img64.numpy())
        changed = int((u8[where] != u8_64[where]).sum())
        print(f'  {n}: {tuple(img.shape)} max {float(img.abs().max()):.3f}; fp32 vs float64 uint8: {changed} entries differ, '
              f'{bad} break the rule', flush=True)
        assert bad == 0, (n, bad)
        others = [i for i in range(len(u8)) if i not in where]
        assert (u8[others] == u8_64[others]).all()
    np.savez_compressed(os.path.join(mg.OUT, 'visual_eval.npz'), **out)
    print('visual_eval.npz', len(out))


def selections():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        paths = vc.write_real_stacks(d)
        vc.seed_pickers()
        out['real_picks'] = vc.picked(ref_ve.Get_Real_Img_Val_Sample(paths, vc.id_transform, vc.REAL_FACES, 'cpu'))
        out['syn_picks'] = vc.picked(ref_ve.Get_Syn_Img_Val_Sample(vc.SynDataset(), vc.SYN_FACES, 'cpu'))
    assert ref_ve.VAL_SET_LEN == vc.VAL_SET_LEN and ref_ve.NUM_IMG_PER_ID == vc.NUM_IMG_PER_ID
    saved = []
    ref_ve.imageio.mimsave = lambda path, frames: saved.append(path)
    single, multi = ref_ve.Get_Single_Photo_Multi_Render_Result, ref_ve.Get_Multi_Photo_Multi_Render_Result
    ref_ve.Get_Single_Photo_Multi_Render_Result = ref_ve.Get_Multi_Photo_Multi_Render_Result = lambda *a, **k: []
    try:
        with tempfile.TemporaryDirectory() as d:
            vc.touch(d, vc.SINGLE_FACTOR_FILES)
            out['single_factor_pairs'] = sorted(list(p) for p in ref_ve.Get_Img_Path_Single_Factor_Test(d))
            ref_ve.Test_Single_Factor_Editing(d, 'SAVE', 'modelA', None, None, 'cpu')
            out['single_factor_results'] = sorted(os.path.relpath(p, 'SAVE') for p in saved)
            del saved[:]
        with tempfile.TemporaryDirectory() as d:
            vc.touch(d, vc.VIDEO_FILES)
            out['video_pairs'] = [list(p) for p in ref_ve.Get_Img_Path_Video_Test(d)]
            ref_ve.Test_Video_Reconstruction_Reanimation(d, 'SAVE', 'clip7', 'modelA', None, None, 'cpu')
            out['video_results'] = [os.path.relpath(p, 'SAVE') for p in saved]
    finally:
        ref_ve.Get_Single_Photo_Multi_Render_Result, ref_ve.Get_Multi_Photo_Multi_Render_Result = single, multi
    # the reference's training script cannot be imported: the names of its checkpoint dict are read off the
    # torch.save call of Sample_Eval_Save_Ckpt
    text = open(os.path.join(mg.REF, 'train_3_encoder.py')).read()
    body = text[text.index('def Sample_Eval_Save_Ckpt'):]
    body = body[body.index('torch.save('):]
    body = body[:body.index('ckpt_dir +')]
    out['checkpoint_keys'] = re.findall(r"^\s*'(\w+)'\s*:", body, flags=re.M)
    assert len(out['checkpoint_keys']) == 14, out['checkpoint_keys']
    with open(os.path.join(mg.OUT, 'visual_eval.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print('visual_eval.json', {k: len(v) for k, v in out.items()})


if __name__ == '__main__':
    selections()
    if '--host-only' not in sys.argv:
        images()
