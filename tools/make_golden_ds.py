#!/usr/bin/env python3
"""Generate tests/golden/train_step_ds.npz: the G phase of a dual-supervision iteration and of an extreme-pose
iteration (train_3_encoder.py:495-558 with ds_flag / extreme_ds_flag set), computed by the imported reference on CPU.

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ds.py
The reference is imported by tools/make_golden.py's recipe (stubs for the CUDA JIT, torchvision and face_alignment).

Per phase (tests/ds_cases.py: DS_CASE, DS_PHASES), with the reference's modules and its own loss functions:
    total = g_nonsaturating_loss(D_edit(fake)) + l1_lambda / shrink * L1_Loss(fake, g_ref)
            + face_lambda * Face_Regional_Loss(r_input, fake)
shrink = ep_lpips_l1_weight_shrink on the extreme-pose batch, else 1; face_lambda = 20 (dual supervision) or 100
(extreme pose).  Stored, fp32 and fp64: the three weighted loss values, the per-sample face scores
(Evaluation/quant_eval.py:167-172), and a strided sample + norm of every G / encoder parameter gradient (packed per
network by tests/ds_cases.py::pack: one zip member per tensor field would triple the file).
"""
import os
import sys

import numpy as np
import torch

import make_golden as MG      # sets up the reference imports; its __main__ is guarded

sys.path.insert(0, os.path.join(MG.ROOT, 'tests'))
import ds_cases  # noqa: E402
import synth  # noqa: E402

stylegan2, network_util, ref_tu = MG.stylegan2, MG.network_util, MG.ref_training_util


def gen_train_step_ds(c=None, fname='train_step_ds.npz'):
    c = c or ds_cases.DS_CASE
    hp, dhp = MG.cases.TRAIN_HP, ds_cases.DS_HP
    out = {}
    size = c['size']
    n_latent = int(np.log2(size)) * 2 - 2
    for dt, sfx in ((torch.float32, ''), (torch.float64, '64')):
        e_tsr, e_w, e_wp = MG.build_encoders(n_latent)
        g = stylegan2.Generator(size, 512, c['n_mlp'])
        g.load_state_dict(synth.state_dict('generator', g.state_dict(), seed=4))
        d_edit = stylegan2.Discriminator(size)
        d_edit.load_state_dict(synth.state_dict('discriminator', d_edit.state_dict(), seed=c['d_edit_seed']))
        ge = dict(g=g, e_tsr=e_tsr, e_w=e_w, e_wp=e_wp)
        for m in list(ge.values()) + [d_edit]:
            m.to(dt)
        for m in ge.values():
            m.requires_grad_(True)
        d_edit.requires_grad_(False)
        wrap = MG._GWrap(g)
        for phase in ds_cases.DS_PHASES:
            extreme = phase == 'ep'
            photo, render = ds_cases.loader_batch(c, phase)
            g_input, r_input, g_ref = (t.to(dt) for t in ds_cases.paired(photo, render, extreme))
            for m in ge.values():
                m.zero_grad(set_to_none=True)
            fake = network_util.Forward_Inference_3_Encoder(g_input, r_input, e_tsr, e_w, e_wp, wrap, 'Photo Image',
                                                            None, False)
            g_loss = ref_tu.g_nonsaturating_loss(d_edit(fake))
            shrink = dhp['ep_lpips_l1_weight_shrink'] if extreme else 1
            l1 = hp['l1_loss_lambda'] / shrink * ref_tu.L1_Loss(fake, g_ref)
            lam = ds_cases.face_lambda(True, extreme)
            face_reg = lam * ref_tu.Face_Regional_Loss(r_input, fake, 'cpu')
            (g_loss + l1 + face_reg).backward()
            with torch.no_grad():
                m_ = ref_tu.Get_Render_Mask(r_input).unsqueeze(1).to(dt)
                scores = torch.mean(torch.square(r_input * m_ - fake * m_), dim=(1, 2, 3))
            p = phase
            out[f'{p}/loss{sfx}'] = np.float64(g_loss.item())
            out[f'{p}/l1{sfx}'] = np.float64(l1.item())
            out[f'{p}/face_reg{sfx}'] = np.float64(face_reg.item())
            out[f'{p}/scores{sfx}'] = MG.npy(scores).astype(np.float64)
            out[f'{p}/mask_frac{sfx}'] = np.float64(float(m_.mean()))
            for k, m in ge.items():
                MG._sample_grads(out, f'{p}/{k}', m.named_parameters(), sfx)
            print('  train_step_ds', p, dt, g_loss.item(), l1.item(), face_reg.item(), flush=True)
            del fake, g_loss, l1, face_reg
    np.savez_compressed(os.path.join(MG.OUT, fname), **ds_cases.pack(out))
    print(fname, len(out))


if __name__ == '__main__':
    os.makedirs(MG.OUT, exist_ok=True)
    torch.manual_seed(0)
    gen_train_step_ds()
