"""Face-regional loss and the dual-supervision iteration (reference Util/training_util.py:228-256,
train_3_encoder.py:495-558 and 777-812).

GPU: the kernel (csrc/face_region.hip) against a float64 restatement of Face_Regional_Loss, mask parity with torch's
`r.mean(1) > -1` on the same device, the G phase of a dual-supervision and an extreme-pose batch against the reference
(tests/golden/train_step_ds.npz, tools/make_golden_ds.py), determinism, no host synchronisation, the schedule of
Trainer.train_iteration, and a reconstruction step that launches nothing new.
CPU: the flag schedule, the weight selection, and the argument checks of the host binding.
"""
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import ds_cases
import launches
import synth
from gpumem import dev, misaligned
from nets import PinNoise, load


# ------------------------------------------------------------------------------------------------------------- CPU
def _tiny_trainer(**over):
    import train_3_encoder as T
    nets = {k: nn.Linear(2, 2) for k in ('G', 'E_Tsr', 'E_W', 'E_W_Plus', 'D', 'D_edit')}
    return T.Trainer(nets, T.default_args(**over))


@pytest.mark.parametrize('ds_freq', [1, 2, 3])
@pytest.mark.parametrize('ex_ds_freq', [1, 3])
def test_ds_flags_follow_reference_loop(ds_freq, ex_ds_freq):
    """Trainer.ds_flags() over 30 iterations == the reference's loop (train_3_encoder.py:780-786), restated."""
    tr = _tiny_trainer(ds_freq=ds_freq, ex_ds_freq=ex_ds_freq)
    got = []
    for _ in range(30):
        got.append(tr.ds_flags())
        tr.iter_idx += 1                    # what step() does at its end
    ref = ds_cases.ds_flags_reference(30, ds_freq, ex_ds_freq)
    assert got == ref
    assert tr.ds_count == sum(f for f, _ in ref)


def test_default_schedule_and_face_lambda():
    """Defaults of train_3_encoder_hyperparams.py:49-50, 69-71 and the weight choice of train_3_encoder.py:521-526."""
    import train_3_encoder as T
    a = T.default_args()
    for k, v in ds_cases.DS_HP.items():
        assert getattr(a, k) == v, k
    for ds_flag, extreme in ((False, False), (True, False), (True, True)):
        assert T.face_reg_lambda(a, ds_flag, extreme) == ds_cases.face_lambda(ds_flag, extreme)
    assert [T.face_reg_lambda(a, *f) for f in ((False, False), (True, False), (True, True))] == [0, 20, 100]
    assert ds_cases.ds_flags_reference(6, 2, 3) == [(False, False), (True, False), (False, False), (True, False),
                                                   (False, False), (True, True)]


def test_shape_mismatch_is_a_value_error_naming_both():
    from op import _native
    from Util.training_util import Face_Regional_Loss
    r, g = torch.zeros(2, 3, 256, 256), torch.zeros(2, 3, 1024, 1024)
    for fn in (lambda: _native.face_region_loss(r, g), lambda: _native.face_region_loss_backward(r, g, torch.ones(())),
               lambda: Face_Regional_Loss(r, g, 'cpu')):
        with pytest.raises(ValueError) as e:
            fn()
        assert '(2, 3, 256, 256)' in str(e.value) and '(2, 3, 1024, 1024)' in str(e.value)
    with pytest.raises(ValueError):
        _native.render_mask(torch.zeros(3, 8, 8))


def test_cpu_tensors_are_refused():
    from op import _native
    from Util.training_util import Face_Regional_Loss, Get_Render_Mask
    r, g = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8)
    for fn in (lambda: _native.face_region_loss(r, g), lambda: _native.face_region_loss_backward(r, g, torch.ones(())),
               lambda: _native.render_mask(r), lambda: Face_Regional_Loss(r, g, 'cpu'), lambda: Get_Render_Mask(r)):
        with pytest.raises(RuntimeError, match='CUDA tensor'):
            fn()


# ------------------------------------------------------------------------------------------------------------- GPU
def _restate64(r, g, m):
    """Face_Regional_Loss (training_util.py:240-256) in float64 for the mask m [B,H,W] (bool): loss, per-sample scores
    (quant_eval.py:172), and d loss / d g."""
    r64, g64 = r.detach().double().cpu(), g.detach().double().cpu()
    mm = m.cpu().unsqueeze(1).double()
    sq = torch.square(r64 * mm - g64 * mm)
    return sq.mean(), sq.mean((1, 2, 3)), 2.0 * (g64 - r64) * mm / r64.numel()


def _run(r, g):
    from op import _native
    from op.face_region import face_region_loss, face_region_scores
    gg = g.detach().requires_grad_(True)          # same storage: a misaligned view stays misaligned
    loss = face_region_loss(r, gg)
    loss.backward()
    return loss.detach(), face_region_scores(r, g), gg.grad, _native.render_mask(r)


SHAPES = [(1, 3, 64, 64), (2, 1, 64, 64), (8, 4, 64, 64),
          (2, 3, 31, 257), (1, 4, 9, 257), (8, 1, 5, 257),
          (8, 3, 64, 1024), (1, 1, 1024, 1024), (2, 4, 32, 1024)]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_matches_fp64_restatement(shape):
    name = 'fr/' + 'x'.join(map(str, shape))
    r = ds_cases.face_render(name + '/r', shape).to(dev())
    g = synth.tensor(name + '/g', shape, dist='uniform').to(dev())
    m = r.mean(1) > -1
    assert 0.1 < float(m.float().mean()) < 0.9
    loss, scores, grad, mask = _run(r, g)
    l64, s64, d64 = _restate64(r, g, m)
    assert abs(float(loss) - float(l64)) <= 1e-5 * abs(float(l64))
    np.testing.assert_allclose(scores.cpu().double().numpy(), s64.numpy(), rtol=1e-5, atol=0)
    assert torch.equal(mask, m.float())
    inside = m.unsqueeze(1).expand(shape).cpu()
    gd = grad.cpu()
    np.testing.assert_allclose(gd[inside].double().numpy(), d64[inside].numpy(), rtol=1e-6, atol=0)
    assert torch.count_nonzero(gd[~inside]) == 0
    # misaligned copies take the scalar form: the same arithmetic in the same order, the same bits
    rv, gv = misaligned(r), misaligned(g)
    loss2, scores2, grad2, mask2 = _run(rv, gv)
    assert torch.equal(loss2, loss) and torch.equal(scores2, scores) and torch.equal(grad2, grad)
    assert torch.equal(mask2, mask)


@pytest.mark.gpu
def test_background_only_render_gives_exact_zeros():
    shape = (2, 3, 64, 64)
    r = torch.full(shape, -1.0, device=dev())
    g = synth.tensor('fr/bg/g', shape, dist='uniform').to(dev())
    loss, scores, grad, mask = _run(r, g)
    assert float(loss) == 0.0 and torch.count_nonzero(scores) == 0
    assert torch.count_nonzero(grad) == 0 and torch.count_nonzero(mask) == 0


@pytest.mark.gpu
def test_non_fp32_gpu_tensors_are_refused():
    from op import _native
    r = torch.zeros(1, 3, 8, 8, device=dev(), dtype=torch.float64)
    with pytest.raises(RuntimeError, match='float32'):
        _native.face_region_loss(r, r)
    with pytest.raises(RuntimeError, match='float32'):
        _native.render_mask(r.half())


def _near_minus_one(k):
    """-1 and its k nearest fp32 neighbours on each side."""
    vals = [np.float32(-1.0)]
    up, down = np.float32(-1.0), np.float32(-1.0)
    for _ in range(k):
        up, down = np.nextafter(up, np.float32(1)), np.nextafter(down, np.float32(-2))
        vals += [up, down]
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize('channels,k', [(3, 6), (4, 4), (1, 6)])
def test_mask_bit_identical_to_torch_mean(channels, k):
    """Every channel tuple (permutations included) of values -1 +- up to k ulp: the HIP decision == torch's
    `r.mean(1) > -1` on the same GPU, in the 16-byte and in the scalar form, and the loss gradient vanishes exactly
    where it is false."""
    from op import _native
    tuples = np.array(list(itertools.product(_near_minus_one(k), repeat=channels)), dtype=np.float32)
    w = 64
    h = -(-len(tuples) // w)
    pix = np.concatenate([tuples, np.repeat(tuples[:1], h * w - len(tuples), 0)])
    r = torch.from_numpy(np.ascontiguousarray(pix.T.reshape(1, channels, h, w))).to(dev())
    ref = (r.mean(1) > -1).float()
    assert 0 < float(ref.sum()) < ref.numel()          # both sides of the boundary are present
    assert torch.equal(_native.render_mask(r), ref)
    assert torch.equal(_native.render_mask(misaligned(r)), ref)
    g = torch.zeros_like(r)
    grad = _native.face_region_loss_backward(r, g, torch.ones((), device=dev()))
    assert torch.equal((grad != 0).any(1).float(), ref)


@pytest.mark.gpu
def test_loss_and_gradient_are_bit_reproducible():
    shape = (4, 3, 256, 256)
    r = ds_cases.face_render('fr/det/r', shape).to(dev())
    g = synth.tensor('fr/det/g', shape, dist='uniform').to(dev())
    a, b = _run(r, g), _run(r, g)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_no_host_synchronisation():
    """Forward and backward under torch.cuda.set_sync_debug_mode('error'), which turns any host synchronisation into
    an error (the reference's term copies its mask to the CPU and back)."""
    from op.face_region import face_region_loss, face_region_scores
    shape = (2, 3, 128, 128)
    r = ds_cases.face_render('fr/sync/r', shape).to(dev())
    g = synth.tensor('fr/sync/g', shape, dist='uniform').to(dev()).requires_grad_(True)
    probe = torch.ones(1, device=dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.item()                     # the mode is live in this build
        loss = 20 * face_region_loss(r, g)
        loss.backward()
        scores = face_region_scores(r, g)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(loss) and g.grad is not None and torch.isfinite(scores).all()


def _ds_nets():
    import stylegan2
    import test_hip_train as H
    c = ds_cases.DS_CASE
    nets = H.build_nets(c['size'], with_d=True, n_mlp=c['n_mlp'])
    nets['d_edit'] = load(stylegan2.Discriminator(c['size']), 'discriminator', c['d_edit_seed'])
    return nets


def _trainer(nets, **over):
    import test_hip_train as H
    import train_3_encoder as T
    return T.Trainer(dict(G=nets['g'], E_Tsr=nets['e_tsr'], E_W=nets['e_w'], E_W_Plus=nets['e_wp'], D=nets['d'],
                          D_edit=nets['d_edit']), H.train_args(**over), dev())


@pytest.mark.gpu
@pytest.mark.parametrize('phase', ds_cases.DS_PHASES)
def test_ds_g_phase_golden(phase, golden):
    """G_Loss_BackProp on a dual-supervision ('ds') and an extreme-pose ('ep') batch vs the reference's modules and loss
    functions (g_nonsaturating_loss on D_edit, L1_Loss with the shrink, Face_Regional_Loss with weight 20 / 100), under
    the gates of test_hip_train.py::test_train_step_phase_golden[...-g]."""
    import dataset
    import test_hip_train as H
    import train_3_encoder as T
    from Util.network_util import Forward_Inference_3_Encoder
    from op.face_region import face_region_scores
    g = ds_cases.Unpacked(golden('train_step_ds'))
    c = ds_cases.DS_CASE
    extreme = phase == 'ep'
    nets = _ds_nets()
    tr = _trainer(nets)
    Dn, d_optim = tr.discriminator(ds_flag=True)
    assert Dn.module is nets['d_edit'] and d_optim is tr.d_edit_optim
    assert tr.discriminator(ds_flag=False)[0].module is nets['d']
    batch = ds_cases.loader_batch(c, phase)
    g_input, r_input, g_ref = dataset.Data_Loading(iter(()), iter([batch]), True, dev(), extreme_loader=iter([batch]),
                                                   extreme_ds_flag=extreme)
    assert g_input.shape[0] == (c['b'] // 2 if extreme else c['b'])
    G = PinNoise(nets['g'], tr.nets['G'])
    ld = {}
    T.G_Loss_BackProp(G, tr.nets['E_Tsr'], tr.nets['E_W'], tr.nets['E_W_Plus'], Dn, g_input, r_input, g_ref, tr.args,
                      ld, None, iter_idx=0, extreme_ds_flag=extreme, ds_flag=True)
    np.testing.assert_allclose(ld['g'].item(), float(g[f'{phase}/loss64']), rtol=1e-4)
    np.testing.assert_allclose(ld['l1'].item(), float(g[f'{phase}/l164']), rtol=1e-4)
    np.testing.assert_allclose(ld['face_reg'].item(), float(g[f'{phase}/face_reg64']), rtol=1e-4)
    kinks = []
    for k in ('g', 'e_tsr', 'e_w', 'e_wp'):
        n, _ = H.check_grads(g, f'{phase}/{k}', nets[k].named_parameters(), kinks=kinks)
        assert n > 20
    H.confirm_kinks(kinks)
    assert all(p.grad is None for p in nets['d'].parameters())           # D is not the one used, and frozen
    assert all(p.grad is None for p in nets['d_edit'].parameters())      # D_edit frozen in the G step
    with torch.no_grad():
        out = Forward_Inference_3_Encoder(g_input, r_input, tr.nets['E_Tsr'], tr.nets['E_W'], tr.nets['E_W_Plus'], G,
                                          'Photo Image', None, False)
    np.testing.assert_allclose(face_region_scores(r_input, out).cpu().numpy(), g[f'{phase}/scores64'], rtol=1e-4)


def _loader(name, b):
    i = 0
    while True:
        yield (synth.tensor(f'{name}/{i}/photo', (b, 3, 256, 256), dist='uniform'),
               ds_cases.face_render(f'{name}/{i}/render', (b, 3, 256, 256)))
        i += 1


@pytest.mark.gpu
def test_train_iteration_schedule_with_d_edit():
    """Six iterations of Trainer.train_iteration at 256^2 with D_edit: flags rec, ds, rec, ds, rec, extreme; D_edit moves
    only in the dual-supervision iterations and D only in the others; the extreme batch is half the size; the
    face-regional term runs (two launches) exactly in the dual-supervision iterations; every loss is finite."""
    nets = _ds_nets()
    tr = _trainer(nets)
    b = 4
    sizes = []
    step = tr.step
    tr.step = lambda g_input, *a, **kw: (sizes.append(g_input.shape[0]), step(g_input, *a, **kw))[1]
    rec, ds, ep = _loader('it/rec', b), _loader('it/ds', b), _loader('it/ep', b)
    flags = []
    for it in range(6):
        before = {k: [p.detach().clone() for p in nets[k].parameters()] for k in ('d', 'd_edit')}
        with launches.observed() as obs:
            ld, ds_flag, extreme = tr.train_iteration(rec, ds, ep)
        flags.append((ds_flag, extreme))
        moved = {k: any(not torch.equal(a, p) for a, p in zip(before[k], nets[k].parameters())) for k in before}
        assert moved == {'d': not ds_flag, 'd_edit': ds_flag}, (it, moved)
        assert obs.count('face_region') == (2 if ds_flag else 0), (it, obs.count('face_region'))
        for k in ('d', 'g', 'l1', 'face_reg', 'r1', 'g_reg'):
            assert torch.isfinite(ld[k]).all(), (it, k)
        assert (float(ld['face_reg'].detach()) > 0) == ds_flag
    assert flags == [(False, False), (True, False), (False, False), (True, False), (False, False), (True, True)]
    assert sizes == [b, b, b, b, b, b // 2]
    assert tr.iter_idx == 6 and tr.ds_count == 3


@pytest.mark.gpu
def test_reconstruction_step_launches_no_face_region_and_mismatch_raises():
    """A default Trainer.step (the reconstruction iteration bench.py times) launches no face_region kernel; a
    dual-supervision step whose renders (256^2) differ in size from the output (64^2) raises the ValueError."""
    import cases
    import test_hip_train as H
    import train_3_encoder as T
    c = cases.TRAIN_STEP_CASE
    nets = H.build_nets(c['size'], with_d=True, n_mlp=2)
    photo, render, ref, _ = H.train_inputs()
    tr = T.Trainer(dict(G=nets['g'], E_Tsr=nets['e_tsr'], E_W=nets['e_w'], E_W_Plus=nets['e_wp'], D=nets['d']),
                   H.train_args(), dev())
    with launches.observed() as obs:
        ld = tr.step(photo, render, ref)
    assert 'face_region' not in obs.names and len(obs.names) > 0
    assert float(ld['face_reg']) == 0.0
    with pytest.raises(ValueError, match=r'\(4, 3, 256, 256\).*\(4, 3, 64, 64\)'):
        tr.step(photo, render, ref, ds_flag=True)
