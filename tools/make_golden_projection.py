#!/usr/bin/env python3
"""Generate tests/golden/projection.npz: the reference's ImageReconstructionLoss, optimize, psnr and
Downsample_Image_256 on the CPU, in fp32 and in float64 (tests/projection_cases.py describes the entries).

Run in the build container only (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_projection.py
The reference is imported as tools/make_golden_ppl.py imports it (JIT, torchvision and `lpips` stubbed; importing that
module does it).  Evaluation/image_projection needs three more substitutions:
  * torchvision.transforms is given Compose / ToTensor / Normalize / Resize / CenterCrop that build nothing (the modules
    compose a transform at import; no image file is read here);
  * the criterion's constructor reads a GPU index from the device string: it is constructed with loss='mse' on 'cpu' and
    then given loss_type, mse_T and `perceptual`, the project's lpips.PerceptualLoss with the weights of
    ppl_cases.percept_state_dict.  forward stays the reference's own;
  * optimize tests the optimiser against `scipy_optim.PyTorchObjective`, a name the reference never imports: the module is
    given a `scipy_optim` whose PyTorchObjective no optimiser is an instance of, so the torch branch is reached.
Inputs and weights come from tests/synth.py on both sides; the file holds OUTPUTS only.
"""
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_ppl as mgp  # noqa: E402  (stubs lpips and model; make_golden stubs the JIT and torchvision)
import projection_cases as pj  # noqa: E402
import ppl_cases as pc  # noqa: E402

mg = mgp.mg
_nothing = lambda *a, **k: None      # noqa: E731
sys.modules['torchvision'].transforms = types.SimpleNamespace(Compose=_nothing, ToTensor=_nothing, Normalize=_nothing,
                                                              Resize=_nothing, CenterCrop=_nothing)
from Evaluation.image_projection import project as ref_project  # noqa: E402
from Evaluation.image_projection import image_projector as ref_projector  # noqa: E402

ref_project.scipy_optim = types.SimpleNamespace(PyTorchObjective=type('PyTorchObjective', (), {}))


def criterion(lp, loss, dt):
    crit = ref_project.ImageReconstructionLoss(device='cpu', loss='mse')
    probe = {'mse': 0.0, 'mse+lpips+mix': 0.01, 'mse+lpips': 100}
    crit.loss_type, crit.mse_T = loss, probe[loss]
    if crit.mse_T > 0.0:
        percept = lp.PerceptualLoss(model='net-lin', net='vgg')
        percept.load_state_dict(pc.percept_state_dict(percept.state_dict()))
        crit.perceptual = percept.to(dt)
    return crit.to(dt)


def run_criterion(c, lp, out):
    res = {}
    for dt in (torch.float32, torch.float64):
        crit = criterion(lp, c['loss'], dt)
        calls = []
        for i in range(len(c['amplitudes'])):
            output, target, mask = pj.criterion_inputs(c, i, dt)
            output.requires_grad_(True)
            loss = crit(output, {'target': target, 'mask': mask})
            loss.backward()
            calls.append((float(loss.detach().double()), output.grad.double(), bool(crit.use_lpips)))
        res[dt] = calls
    for i, ((l32, g32, u32), (l64, g64, u64)) in enumerate(zip(res[torch.float32], res[torch.float64])):
        assert u32 == u64
        k = f"{c['name']}/{i}/"
        s = c['stride']
        out[k + 'loss'], out[k + 'loss64'] = np.float64(l32), np.float64(l64)
        out[k + 'grad64'] = g64[:, :, ::s, ::s].numpy()
        out[k + 'grad_max64'] = np.float64(g64.abs().max())
        out[k + 'grad_err'] = np.float64((g32 - g64).abs().max())
        out[k + 'use_lpips'] = np.bool_(u64)
        print(f"  {k} loss {l32:.9e} / {l64:.9e} rel {abs(l32 - l64) / abs(l64):.2e} grad err/max "
              f"{float(out[k + 'grad_err']) / float(out[k + 'grad_max64']):.2e} lpips {u64}", flush=True)


def generator(c, dt):
    if c['kind'] == 'toy':
        return pj.ToyProjGenerator().to(dt)
    g = mg.stylegan2.Generator(c['size'], pj.LATENT_DIM, 2, channel_multiplier=1)
    g.load_state_dict(mg.synth.state_dict('generator', g.state_dict(), seed=4))
    return g.to(dt).eval().requires_grad_(False)


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def run_trajectory(c, lp, out):
    res = {}
    for dt in (torch.float32, torch.float64):
        g = generator(c, dt)
        avg_w, noises, target = pj.trajectory_start(c, g, dt)
        start = [avg_w.clone()] + [n.clone() for n in noises]
        avg_w.requires_grad = True
        for n in noises:
            n.requires_grad = True
        crit = criterion(lp, 'mse+lpips', dt)
        optimizer = torch.optim.Adam([avg_w] + noises, lr=pj.LR)
        lrs, losses = [], []
        seen = crit.forward

        def recording(output, targets, **kw):
            loss = seen(output, targets, **kw)
            lrs.append(optimizer.param_groups[0]['lr'])
            losses.append(float(loss.detach().double()))
            return loss
        crit.forward = recording
        kwargs = {'noise_z': None, 'input_is_latent': True, 'latent_styles': [avg_w], 'noise': noises}
        ref_project.optimize(model=g, input_kwargs=kwargs, targets={'target': target, 'mask': None}, criterion=crit,
                             optimizer=optimizer, iterations=c['iterations'], print_iterations=10 ** 6, device='cpu')
        disp = [(p.detach() - s).double() for p, s in zip([avg_w] + noises, start)]
        res[dt] = dict(lr=np.array(lrs), loss=np.array(losses), disp=disp)
    r32, r64 = res[torch.float32], res[torch.float64]
    n = c['name']
    assert len(r64['lr']) == c['iterations'] + 1 and np.array_equal(r32['lr'], r64['lr'])
    out[n + '/lr'], out[n + '/loss'], out[n + '/loss64'] = r64['lr'], r32['loss'], r64['loss']
    errs = [rel_l2(a, b) for a, b in zip(r32['disp'], r64['disp'])]
    out[n + '/dW64'] = r64['disp'][0].numpy()
    for i, d in enumerate(r64['disp'][1:]):
        out[f'{n}/dnoise{i}64'] = pj.noise_sample(d).numpy()
    out[n + '/dW_err'], out[n + '/dnoise_err'] = np.float64(errs[0]), np.array(errs[1:])
    loss_rel = np.abs(r32['loss'] - r64['loss']) / np.abs(r64['loss'])
    print(f"  {n}: lr {r64['lr']} loss64 {r64['loss']} rel loss err {loss_rel.max():.2e} dW err {errs[0]:.2e} "
          f"dnoise err max {max(errs[1:]):.2e}", flush=True)
    assert loss_rel.max() <= 1e-2 and max(errs) <= 1e-2, \
        f'{n}: the fp32 run leaves its float64 run by more than 1e-2: reduce the iterations in tests/projection_cases.py'


def run_helpers(out):
    for i in range(2):
        a, b = pj.image_pair(i)
        out[f'helpers/psnr/{i}'] = np.float64(ref_projector.psnr(pj.to_255(a), pj.to_255(b)))
        out[f'helpers/down/{i}'] = ref_projector.Downsample_Image_256(pj.down_input(i))[:, :, ::9, ::9].numpy()
    a, _ = pj.image_pair(0)
    out['helpers/psnr/equal'] = np.float64(ref_projector.psnr(pj.to_255(a), pj.to_255(a)))


def main():
    lp = mgp.project_lpips()
    out = {}
    for c in pj.CRITERION_CASES:
        t = time.time()
        run_criterion(c, lp, out)
        print(f"  {c['name']}: {time.time() - t:.1f} s", flush=True)
    for c in pj.TRAJECTORIES:
        t = time.time()
        run_trajectory(c, lp, out)
        print(f"  {c['name']}: {time.time() - t:.1f} s", flush=True)
    run_helpers(out)
    path = os.path.join(mg.OUT, 'projection.npz')
    np.savez_compressed(path, **out)
    print('projection', len(out), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
