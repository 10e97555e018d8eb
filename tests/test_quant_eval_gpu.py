"""GPU tests of the quantitative evaluation (Evaluation/quant_eval.py, Trainer.evaluate): the three cases of
tests/quant_eval_cases.py per sample against the reference's values (tests/golden/quant_eval.npz), fused and baseline
form; LPIPS through the real PerceptualLoss; Trainer.evaluate leaves the training state alone."""

import numpy as np
import pytest
import torch

import quant_eval_cases as qc
import synth
from gpumem import dev
from nets import PinNoise
from test_hip_train import build_nets, train_args

pytestmark = pytest.mark.gpu

# Floors (absolute) of the cosine-similarity and stand-in-distance gates: see test_scores_golden.
COS_FLOOR, DIST_FLOOR = 5e-7, 6.6e-5


@pytest.fixture(scope='module')
def nets256():
    n = build_nets(256)
    from Util.arcface_pytorch.resnet_face_recognition import resnet_face18
    arc = resnet_face18(use_se=False)
    arc.load_state_dict(synth.state_dict('arcface', arc.state_dict(), seed=9))
    n['arc'] = arc.eval().requires_grad_(False).to(dev())
    return n


def _standin_distance(x, y):
    return ((x - y) ** 2).mean([1, 2, 3]).view(-1, 1, 1, 1)


def _scores(c, nets, fuse, monkeypatch):
    from Evaluation import quant_eval as QE
    monkeypatch.setattr(QE, 'EVAL_FUSE', fuse)
    fwd = dict(tsr_encode=c['tsr_encode'], sliced_layer=c['sliced_layer'], use_tanh=c['use_tanh'])
    enc = (nets['e_tsr'], nets['e_w'], nets['e_wp'])
    if c['kind'] == 'recon':
        # Forward_Inference_3_Encoder passes no noise arguments: the wrapper pins the stored noise, as the fixture's did
        return QE.Recon_Scores(qc.recon_loader(c), dev(), enc + (PinNoise(nets['g']),), (nets['arc'], _standin_distance),
                               **fwd)
    return QE.Edit_Scores(qc.edit_loader(c), dev(), enc + (nets['g'],), (nets['arc'], None, None),
                          randomize_noise=False, **fwd)


@pytest.mark.parametrize('fuse', [True, False], ids=['fused', 'baseline'])
@pytest.mark.parametrize('c', qc.QUANT_EVAL_CASES, ids=lambda c: c['name'])
def test_scores_golden(c, fuse, golden, nets256, monkeypatch):
    """Per sample against the float64 fixture.
      l1         |d| <= 5e-5 * max|image|: the project's end-to-end image gate; a mean of absolute differences is
                 1-Lipschitz in the sup norm.
      face_diff  rtol 1e-4, the gate test_face_region.py holds scores64 to.
      cos, dist  |d| <= 4 * |reference fp32 - reference fp64| + floor.  The reference's own difference (cos 2e-8 .. 1.3e-7,
                 stand-in distance 7e-6 .. 2.2e-5 on values of 24 .. 32) comes from three or four samples, too few to bound
                 this path's; the floor is twice the largest difference from the float64 fixture measured on the MI355X
                 over the three cases, both forms, three runs (profiles/quant_eval.md): cos 2.49e-7 -> 5e-7, stand-in distance
                 3.31e-5 -> 6.6e-5.
    Each figure is printed before it is asserted."""
    g = golden('quant_eval')
    s = _scores(c, nets256, fuse, monkeypatch)
    n = c['name']
    keys = ('cos', 'lpips', 'l1') if c['kind'] == 'recon' else ('cos', 'face_diff')
    got = {k: s[k].double().cpu().numpy() for k in keys}
    for k in keys:
        ref32, ref64 = g[f'{n}/{k}'], g[f'{n}/{k}64']
        assert got[k].shape == ref64.shape, k
        d = np.abs(got[k] - ref64)
        print(f'{n} {"fused" if fuse else "baseline"} {k}: max|d| {d.max():.3e} rel {np.max(d / np.abs(ref64)):.3e} '
              f'reference fp32-fp64 {np.abs(ref32 - ref64).max():.3e}')
    for k in keys:
        ref32, ref64 = g[f'{n}/{k}'], g[f'{n}/{k}64']
        d = np.abs(got[k] - ref64)
        if k == 'l1':
            assert np.all(d <= 5e-5 * float(g[f'{n}/absmax64'])), (k, d)
        elif k == 'face_diff':
            np.testing.assert_allclose(got[k], ref64, rtol=1e-4, atol=0)
        else:
            floor = COS_FLOOR if k == 'cos' else DIST_FLOOR
            assert np.all(d <= 4 * np.abs(ref32 - ref64) + floor), (k, d)


def test_get_scores_return_the_reference_tuples(golden, nets256, monkeypatch):
    """Get_Recon_Score / Get_Edit_Score on the first two cases: the reference's 3- and 5-tuples of float64 means, within
    the per-sample gates of test_scores_golden applied to the means."""
    from Evaluation import quant_eval as QE
    g = golden('quant_eval')
    c = qc.QUANT_EVAL_CASES[0]
    enc = (nets256['e_tsr'], nets256['e_w'], nets256['e_wp'])
    out = QE.Get_Recon_Score(qc.recon_loader(c), dev(), enc + (PinNoise(nets256['g']),), (nets256['arc'], _standin_distance),
                             tsr_encode=c['tsr_encode'])
    m32, m64 = g[c['name'] + '/means'], g[c['name'] + '/means64']
    assert len(out) == 3 and all(isinstance(v, np.float64) for v in out)
    assert abs(out[0] - m64[0]) <= 4 * abs(m32[0] - m64[0]) + COS_FLOOR
    assert abs(out[1] - m64[1]) <= 4 * abs(m32[1] - m64[1]) + DIST_FLOOR
    assert abs(out[2] - m64[2]) <= 5e-5 * float(g[c['name'] + '/absmax64'])
    c = qc.QUANT_EVAL_CASES[1]
    out = QE.Get_Edit_Score(qc.edit_loader(c), dev(), enc + (nets256['g'],), (nets256['arc'], None, None),
                            tsr_encode=c['tsr_encode'], randomize_noise=False)
    m32, m64 = g[c['name'] + '/means'], g[c['name'] + '/means64']
    assert len(out) == 5 and out[1:4] == (None, None, None)
    assert abs(out[0] - m64[0]) <= 4 * abs(m32[0] - m64[0]) + COS_FLOOR
    np.testing.assert_allclose(out[4], m64[1], rtol=1e-4)


def test_recon_lpips_is_the_perceptual_loss_of_the_same_images(nets256, monkeypatch):
    """Get_Recon_Score's LPIPS with the real lpips.PerceptualLoss at [2,3,256,256]: per sample the module's own output on
    the images the loop produced (they are recorded: the encoders' library convolutions need not repeat bit for bit).  The
    VGG trunk's convolutions are library kernels too, hence rtol 1e-5 instead of equality."""
    import lpips
    from Evaluation import quant_eval as QE
    percept = lpips.PerceptualLoss(model='net-lin', net='vgg').to(dev())
    c = qc.QUANT_EVAL_CASES[0]
    loader = qc.recon_loader(c)[:1]
    seen = []
    forward = QE.Forward_Inference_3_Encoder

    def recording(*a, **kw):
        seen.append(forward(*a, **kw).clone())
        return seen[-1]
    monkeypatch.setattr(QE, 'Forward_Inference_3_Encoder', recording)
    s = QE.Recon_Scores(loader, dev(), (nets256['e_tsr'], nets256['e_w'], nets256['e_wp'], PinNoise(nets256['g'])),
                        (nets256['arc'], percept))
    assert len(seen) == 1 and tuple(seen[0].shape) == (2, 3, 256, 256) and tuple(s['lpips'].shape) == (2,)
    with torch.no_grad():
        direct = percept(seen[0], loader[0][0].to(dev())).reshape(-1)
    torch.testing.assert_close(s['lpips'], direct, rtol=1e-5, atol=0)
    assert bool((s['lpips'] > 0).all())


# ------------------------------------------------------------------------------------------------ Trainer.evaluate
KEYS = ('cos_score', 'lpips_score', 'l1_score', 'cos_score_edit', 'fid', 'hmap_score', 'lmark_score', 'face_reg_score')


def _state(tr, nets):
    mods = dict(nets, g_ema=tr.g_ema)
    params = {f'{k}/{n}': t.detach().clone() for k, m in mods.items() for n, t in m.state_dict().items()}
    flags = {f'{k}/{n}': p.requires_grad for k, m in mods.items() for n, p in m.named_parameters()}
    training = {f'{k}/{n}': sub.training for k, m in mods.items() for n, sub in m.named_modules()}
    optim = {}
    for name in ('g_enc_optim', 'd_optim'):
        for i, st in enumerate(getattr(tr, name).state.values()):
            for key, v in st.items():
                optim[f'{name}/{i}/{key}'] = v.detach().clone() if torch.is_tensor(v) else v
    return params, flags, training, optim


def test_trainer_evaluate_leaves_the_training_state_alone(nets256):
    """Trainer.evaluate on copies of this module's 256^2 networks plus Discriminator(256): the evaluation compares outputs
    with 256^2 photos pixel by pixel, so the 64^2 generator of test_hip_train.py's Trainer does not apply.  To keep the
    test short the encoders are frozen (tsr_train / w_train / w_plus_train off: no backward through them in the step that
    follows) and the perceptual term is a stand-in distance (the real module is the subject of the test above).  Checked:
    the reference's log names; every parameter, buffer and optimiser-state tensor bit-unchanged; requires_grad,
    .training and the counters unchanged; a step() afterwards still runs."""
    import copy
    import stylegan2
    import train_3_encoder as T
    nets = dict(G=copy.deepcopy(nets256['g']), E_Tsr=copy.deepcopy(nets256['e_tsr']), E_W=copy.deepcopy(nets256['e_w']),
                E_W_Plus=copy.deepcopy(nets256['e_wp']), D=stylegan2.Discriminator(256))
    nets['D'].load_state_dict(synth.state_dict('discriminator', nets['D'].state_dict(), seed=8))
    nets['D'].to(dev())
    args = train_args(tsr_train=False, w_train=False, w_plus_train=False)
    tr = T.Trainer(nets, args, dev(), lpips_model=lambda x, y: _standin_distance(x, y).reshape(-1),
                   face_rec_model=nets256['arc'])
    # optimiser state without the cost of an iteration: one Adam step on small constant gradients
    for opt in (tr.g_enc_optim, tr.d_optim):
        for grp in opt.param_groups:
            for p in grp['params']:
                p.grad = torch.full_like(p, 1e-3)
        opt.step()
        opt.zero_grad(set_to_none=True)
    nets['G'].train()
    nets['D'].train()
    tr.iter_idx, tr.ds_count, tr.mean_path_length = 5, 2, torch.tensor(0.375, device=dev())
    before = _state(tr, nets)
    assert len(before[3]) > 100

    c = qc.QUANT_EVAL_CASES[1]
    rec = qc.recon_loader(qc.QUANT_EVAL_CASES[0])[:1]
    scores = tr.evaluate(rec, qc.edit_loader(c))
    assert tuple(scores) == KEYS
    for k in ('cos_score', 'lpips_score', 'l1_score', 'cos_score_edit', 'face_reg_score'):
        assert isinstance(scores[k], np.float64) and np.isfinite(scores[k]), k
    assert scores['fid'] is None and scores['hmap_score'] is None and scores['lmark_score'] is None
    assert -1.0 <= scores['cos_score'] <= 1.0 and scores['l1_score'] > 0 and scores['face_reg_score'] > 0
    only_rec = tr.evaluate(rec_eval_loader=rec)
    assert tuple(only_rec) == KEYS and only_rec['cos_score_edit'] is None and only_rec['face_reg_score'] is None
    assert only_rec['l1_score'] > 0

    after = _state(tr, nets)
    for b, a in zip(before[:3], after[:3]):
        assert b.keys() == a.keys()
    assert all(torch.equal(before[0][k], after[0][k]) for k in before[0])
    assert before[1] == after[1] and before[2] == after[2]
    assert nets['G'].training and nets['D'].training and not tr.g_ema.training and not nets['E_W_Plus'].training
    assert before[3].keys() == after[3].keys()
    for k, v in before[3].items():
        assert torch.equal(v, after[3][k]) if torch.is_tensor(v) else v == after[3][k], k
    assert tr.iter_idx == 5 and tr.ds_count == 2 and float(tr.mean_path_length) == 0.375
    assert all(p.grad is None for m in nets.values() for p in m.parameters())

    photo, render = (t.to(dev()) for t in rec[0])
    ld = tr.step(photo, render, photo.clone())                # iteration 5: no R1, no path-length step
    assert tr.iter_idx == 6 and all(torch.isfinite(ld[k]).all() for k in ('d', 'g', 'l1', 'lpips', 'face_id'))
