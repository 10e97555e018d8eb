#!/usr/bin/env python3
"""Generate tests/golden/quant_eval.npz: reconstruction and editing scores by the reference on CPU.

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_quant_eval.py
The reference is imported exactly as tools/make_golden.py imports it (JIT and torchvision stubbed; importing that
module does it).  Two more stubs are needed for Evaluation/quant_eval.py: `Evaluation.fid` (scipy-based, only calc_fid is
imported) and Get_HeatMap_Landmark_PyTorch of the already stubbed Util.landmark_util (face_alignment is absent).

  recon cases  the reference's own Get_Recon_Score.  Its per-sample lists never leave the function, so the module's `np`
               is replaced for the call by a recorder whose `mean` notes each list before averaging it.  The `lpips`
               package cannot be imported offline: a stand-in distance ((x - y)^2).mean([1,2,3]) takes its place.
  edit cases   Get_Edit_Score unconditionally opens an Inception statistics file that is not shipped and calls the
               landmark network, so its loop is restated here from the reference's own pieces: Forward_Inference_3_Encoder
               per render, Get_Render_Mask and the three face-difference lines (quant_eval.py:167-172), then
               Compute_Face_Identity_Similarity on the list of outputs (quant_eval.py:187-189).
Networks: make_golden.build_encoders(14), Generator(256, 512, 8) seed 4, ArcFace seed 9; _GWrap pins the noise.  Each case
runs in fp32 and in float64.  Inputs and weights come from tests/synth.py on both sides; the file holds OUTPUTS only: per
case the per-sample values (`/cos`, `/lpips`, `/l1`, `/face_diff`), their means (`/means`), the float64 run's (`...64`)
and the largest |pixel| the generator produced, before any tanh (`/absmax`); `identity_256/cos` is Compute_Face_Identity_Similarity alone, [output, sample].
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (stubs the JIT, puts the reference and tests/ on sys.path)
import quant_eval_cases as qc  # noqa: E402

sys.modules['Util.landmark_util'].Get_HeatMap_Landmark_PyTorch = None
_fid = types.ModuleType('Evaluation.fid'); _fid.calc_fid = None
sys.modules['Evaluation.fid'] = _fid
from Evaluation import quant_eval as ref_qe  # noqa: E402
from Util.arcface_pytorch.resnet_face_recognition import resnet_face18  # noqa: E402


def standin_distance(x, y):
    return ((x - y) ** 2).mean([1, 2, 3]).view(-1, 1, 1, 1)


class _Recorder:
    """Stands in for numpy inside the reference module: mean() keeps the list it averages."""

    def __init__(self):
        self.lists = []

    def mean(self, values):
        self.lists.append(np.asarray(values, dtype=np.float64))
        return np.mean(values)


class _AbsMax:
    """_GWrap that also notes the largest |pixel| it produced."""

    def __init__(self, g):
        self.module, self.absmax = g, 0.0

    def __call__(self, **kw):
        out = self.module(randomize_noise=False, **kw)
        self.absmax = max(self.absmax, float(out.abs().max()))
        return out


def networks(dt):
    e_tsr, e_w, e_wp = mg.build_encoders(14)
    g = mg.stylegan2.Generator(256, 512, 8)
    g.load_state_dict(mg.synth.state_dict('generator', g.state_dict(), seed=4))
    g.eval()
    arc = resnet_face18(use_se=False)
    arc.load_state_dict(mg.synth.state_dict('arcface', arc.state_dict(), seed=9))
    arc.eval().requires_grad_(False)
    for m in (e_tsr, e_w, e_wp, g, arc):
        m.to(dt)
    return e_tsr, e_w, e_wp, g, arc


def run_recon(c, dt):
    e_tsr, e_w, e_wp, g, arc = networks(dt)
    wrap = _AbsMax(g)
    loader = [(p.to(dt), r.to(dt)) for p, r in qc.recon_loader(c)]
    rec, orig = _Recorder(), ref_qe.np
    try:
        ref_qe.np = rec
        means = ref_qe.Get_Recon_Score(loader, 'cpu', (e_tsr, e_w, e_wp, wrap), (arc, standin_distance),
                                       tsr_encode=c['tsr_encode'], sliced_layer=c['sliced_layer'],
                                       use_tanh=c['use_tanh'])
    finally:
        ref_qe.np = orig
    cos, lp, l1 = rec.lists
    return dict(cos=cos, lpips=lp.reshape(-1), l1=l1, means=np.asarray(means, dtype=np.float64), absmax=wrap.absmax)


def run_edit(c, dt):
    e_tsr, e_w, e_wp, g, arc = networks(dt)
    wrap = _AbsMax(g)
    cos, face_diff = [], []
    for batch in qc.edit_loader(c):
        p_input = batch[0].to(dt)
        g_output_list = []
        for r_input in batch[1:]:
            r_input = r_input.to(dt)
            g_output = mg.network_util.Forward_Inference_3_Encoder(p_input, r_input, e_tsr, e_w, e_wp, wrap,
                                                                   tsr_encode=c['tsr_encode'],
                                                                   sliced_layer=c['sliced_layer'], use_tanh=c['use_tanh'])
            g_output_list.append(g_output)
            mask_unsqueeze = mg.ref_training_util.Get_Render_Mask(r_input).unsqueeze(1)
            masked_r, masked_g = r_input * mask_unsqueeze, g_output * mask_unsqueeze
            face_diff += torch.mean(torch.square(masked_r - masked_g), dim=(1, 2, 3)).tolist()
        for s in ref_qe.Compute_Face_Identity_Similarity(g_output_list, p_input, arc):
            cos += s.tolist()
    cos, face_diff = np.asarray(cos, dtype=np.float64), np.asarray(face_diff, dtype=np.float64)
    return dict(cos=cos, face_diff=face_diff, means=np.array([cos.mean(), face_diff.mean()]), absmax=wrap.absmax)


def run_identity(dt):
    """The reference's Compute_Face_Identity_Similarity in its tensor and its list form."""
    arc = networks(dt)[-1]
    target, outs = qc.identity_inputs()
    target, outs = target.to(dt), [o.to(dt) for o in outs]
    single = ref_qe.Compute_Face_Identity_Similarity(outs[0], target, arc)
    listed = ref_qe.Compute_Face_Identity_Similarity(outs, target, arc)
    assert torch.equal(single, listed[0])
    return np.stack([s.numpy().astype(np.float64) for s in listed])


def main():
    out = {}
    with torch.no_grad():
        for dt, sfx in ((torch.float32, ''), (torch.float64, '64')):
            out[qc.IDENTITY_CASE['name'] + '/cos' + sfx] = run_identity(dt)
            print(' ', qc.IDENTITY_CASE['name'], dt, out[qc.IDENTITY_CASE['name'] + '/cos' + sfx].tolist(), flush=True)
        for c in qc.QUANT_EVAL_CASES:
            run = run_recon if c['kind'] == 'recon' else run_edit
            for dt, sfx in ((torch.float32, ''), (torch.float64, '64')):
                res = run(c, dt)
                for k, v in res.items():
                    out[f"{c['name']}/{k}{sfx}"] = np.asarray(v, dtype=np.float64)
                print(' ', c['name'], dt, {k: np.asarray(v).tolist() for k, v in res.items()}, flush=True)
    np.savez_compressed(os.path.join(mg.OUT, 'quant_eval.npz'), **out)
    print('quant_eval', len(out))


if __name__ == '__main__':
    main()
