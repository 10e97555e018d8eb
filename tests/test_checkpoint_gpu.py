"""GPU tests of the Trainer's checkpoints and of Sample_Eval_Save_Ckpt, on the smallest Trainer the training tests build
(tests/cases.py TRAIN_STEP_CASE: Generator(64, 512, n_mlp=2), Discriminator(64), 256^2 photos) with a second
Discriminator(64) as D_edit, at B = 2; renders and targets at the output's size, so that a dual-supervision iteration
(face-regional term) runs.

One module fixture trains three iterations — a reconstruction iteration with the R1 and the path-length step, a
dual-supervision one, a reconstruction one — calling Sample_Eval_Save_Ckpt after each with val_sample_freq =
model_save_freq = 2; the tests share its files and its final state and leave both unchanged.

Continuation: training on MIOpen is not bit-reproducible, so iteration 4 is run twice from two deep copies
of the state after iteration 3; the largest relative difference between the two over all parameters is the run-to-run
spread of the training code itself (printed; profiles/visual_eval.md), and the resumed Trainer's iteration 4 must agree
with the first copy within 4 x that spread (parity.within_reference's margin), with a floor of 1e-6 of each tensor's max.
A load that dropped Adam's moments or the EMA misses this by orders of magnitude."""
import copy
import io
import os

import numpy as np
import pytest
import torch

import cases
import ds_cases
import synth
import visual_eval_cases as vc
from gpumem import dev
from nets import load

pytestmark = pytest.mark.gpu
B = 2
SIZE = cases.TRAIN_STEP_CASE['size']
NETS = ('G', 'E_Tsr', 'E_W', 'E_W_Plus', 'D', 'D_edit')
SCORES = dict(cos_score=0.5, lpips_score=0.25, l1_score=0.125, cos_score_edit=0.75, fid=12.5, hmap_score=None,
              lmark_score=None, face_reg_score=0.0625)


def _nets(seed_shift=0):
    """The networks of tests/test_hip_train.py::build_nets(64) and a D_edit; seed_shift != 0: other weights of the same
    shapes."""
    import types
    import resnet_encoder
    import stylegan2
    from psp_encoder_model.encoders import psp_encoders
    c = dict(ds_cases.DS_CASE, size=SIZE)
    n_latent = int(np.log2(c['size'])) * 2 - 2
    s = seed_shift
    return dict(
        G=load(stylegan2.Generator(c['size'], 512, c['n_mlp']), 'generator', 4 + s),
        E_Tsr=load(resnet_encoder.resnet18(tensor_encoding=True, tensor_transform=False), 'resnet', 5 + s),
        E_W=load(resnet_encoder.resnet18(tensor_encoding=False, tensor_transform=False), 'resnet', 6 + s),
        E_W_Plus=load(psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=n_latent)),
                      'psp', 7 + s),
        D=load(stylegan2.Discriminator(c['size']), 'discriminator', c['d_seed'] + s),
        D_edit=load(stylegan2.Discriminator(c['size']), 'discriminator', c['d_edit_seed'] + s))


def _trainer(seed_shift=0):
    import test_hip_train as H
    import train_3_encoder as T
    return T.Trainer(_nets(seed_shift), H.train_args(val_sample_freq=2, model_save_freq=2, val_sample_tile=SIZE), dev())


def _iterate(tr, it):
    """Iteration `it` of the schedule (the flags as train_iteration draws them) on its own fixed batch, the generator's
    noise seeded and the path-length sample fixed.  Returns (ds_flag, extreme_ds_flag)."""
    torch.manual_seed(100 + it)
    photo = synth.tensor(f'ckpt/{it}/photo', (B, 3, 256, 256), dist='uniform').to(dev())
    render = ds_cases.face_render(f'ckpt/{it}/render', (B, 3, SIZE, SIZE)).to(dev())
    ref = synth.tensor(f'ckpt/{it}/ref', (B, 3, SIZE, SIZE), dist='uniform').to(dev())
    ds_flag, extreme = tr.ds_flags()
    tr.step(photo, render, ref, ppl_choice=[1], ds_flag=ds_flag, extreme_ds_flag=extreme)
    return ds_flag, extreme


def _copy(tr):
    """copy.deepcopy of a Trainer: its loss_dict holds the last iteration's graph tensors, which deepcopy refuses."""
    kept = tr.loss_dict
    tr.loss_dict = {k: v.detach() for k, v in kept.items()}
    try:
        return copy.deepcopy(tr)
    finally:
        tr.loss_dict = kept


def _modules(tr):
    return [(k, tr.bare[k]) for k in NETS] + [('g_ema', tr.g_ema)]


def _tensors(tr):
    """Every parameter and buffer of every network and of g_ema, by name."""
    return {f'{k}/{n}': t for k, m in _modules(tr) for n, t in m.state_dict().items()}


def _optim_state(tr):
    """Every state tensor and step count of the three optimisers, by (optimiser, parameter position, field)."""
    out = {}
    for name in ('g_enc_optim', 'd_optim', 'd_edit_optim'):
        sd = getattr(tr, name).state_dict()
        out[name + '/groups'] = [{k: v for k, v in g.items()} for g in sd['param_groups']]
        for idx, st in sd['state'].items():
            for field, v in st.items():
                out[f'{name}/{idx}/{field}'] = v
    return out


def _same(a, b):
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


@pytest.fixture(scope='module')
def fresh():
    """A Trainer from other weights of the same shapes; every test loads a checkpoint into it first."""
    return _trainer(seed_shift=50)


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    root = tmp_path_factory.mktemp('run')
    sample_dir, ckpt_dir = str(root / 'sample'), str(root / 'ckpt')
    tr = _trainer()
    samples = [t.to(dev()) for t in vc.batch_inputs(dict(vc.BATCH, name='ckpt/samples', sets=1))]
    flags, returned, log = [], [], io.StringIO()
    for it in range(3):
        flags.append(_iterate(tr, it))
        if it == 2:             # the quantitative half with stand-in scores: its log text, without the loss networks
            tr.evaluate = lambda rec, edit: dict(SCORES)
        try:
            returned.append(tr.Sample_Eval_Save_Ckpt(sample_dir, ckpt_dir, samples, rec_eval_loader=[], edit_eval_loader=[],
                                                     log=log))
        finally:
            tr.__dict__.pop('evaluate', None)
    return dict(tr=tr, sample_dir=sample_dir, ckpt_dir=ckpt_dir, flags=flags, returned=returned, log=log.getvalue(),
                samples=samples)


def test_sample_eval_save_ckpt_writes_the_expected_files(trained):
    """val_sample_freq = model_save_freq = 2 over iterations 0, 1, 2: sheets for 0 and 2, a checkpoint for 2 only (none at
    iteration 0), the reference's names; the sheet on disk is Trainer.sample's; the log carries the reference's text."""
    Image = pytest.importorskip('PIL.Image')
    tr = trained['tr']
    assert trained['flags'] == [(False, False), (True, False), (False, False)]
    assert tr.iter_idx == 3 and tr.ds_count == 1 and float(tr.mean_path_length) > 0
    assert sorted(os.listdir(trained['sample_dir'])) == ['000000.png', '000002.png']
    assert sorted(os.listdir(trained['ckpt_dir'])) == ['000002.pt']
    png = [r[0] and os.path.basename(r[0]) for r in trained['returned']]
    ckpt = [r[2] and os.path.basename(r[2]) for r in trained['returned']]
    assert png == ['000000.png', None, '000002.png'] and ckpt == [None, None, '000002.pt']
    assert [r[1] for r in trained['returned']] == [None, None, SCORES]
    assert trained['log'] == ('\nReconstruction Quantitative Evaluation: \nCosine Similarity: 0.5\nLPIPS Score: 0.25\n'
                              'L1 Score: 0.125\n\nEdit Quantitative Evaluation: \nEdit Cosine Similarity: 0.75\nFID: 12.5\n'
                              'Heat Map: None\nLand Mark: None\nFace Regional: 0.0625\n\n')
    # the sheet: one set -> one row of five tiles of the output's size, gap and margin 8
    flags = [m.training for _, net in _modules(tr) for m in net.modules()]
    torch.manual_seed(5)
    sheet = tr.sample(trained['samples'], tile=SIZE, randomize_noise=False)
    assert flags == [m.training for _, net in _modules(tr) for m in net.modules()]      # every training flag restored
    assert sheet.dtype == torch.uint8 and tuple(sheet.shape) == (16 + SIZE, 16 + 5 * SIZE + 4 * 8, 3) and sheet.is_cuda
    with Image.open(os.path.join(trained['sample_dir'], '000002.png')) as img:
        disk = np.asarray(img.convert('RGB'))
    assert disk.shape == tuple(sheet.shape)
    host = sheet.cpu().numpy()
    photo = (slice(8, 8 + SIZE), slice(8, 8 + SIZE))        # the photo and the renders do not depend on the noise
    np.testing.assert_array_equal(disk[photo], host[photo])
    assert (disk[:8] == 255).all() and (disk[:, 8 + SIZE:16 + SIZE] == 255).all()
    assert (disk[8:8 + SIZE, 24 + 2 * SIZE:24 + 3 * SIZE] != 255).any()      # the first output's tile was written


def test_checkpoint_round_trip(trained, fresh):
    """save_checkpoint's file into a fresh Trainer built from other weights: every parameter and buffer of every network
    and of g_ema, every optimiser state tensor and step count, the three counters and the next four ds_flags() equal."""
    tr = trained['tr']
    path = os.path.join(trained['ckpt_dir'], '000002.pt')
    want = _tensors(tr)
    other = _tensors(_trainer(seed_shift=50)) if fresh.iter_idx else _tensors(fresh)     # as built, before any load
    assert want.keys() == other.keys() and sum(not torch.equal(want[k], other[k]) for k in want) > 0.5 * len(want)
    del other
    wrapped = {k: fresh.nets[k] for k in NETS}
    ck = fresh.load_checkpoint(path)
    assert list(ck)[-1] == 'trainer' and len(ck) == 15
    got = _tensors(fresh)
    assert [k for k in want if not torch.equal(want[k], got[k])] == []
    for k in NETS:                                           # the wrapped networks are the ones that were loaded
        assert fresh.nets[k] is wrapped[k] and fresh.nets[k].module is fresh.bare[k]
    a, b = _optim_state(tr), _optim_state(fresh)
    assert a.keys() == b.keys() and len(a) > 100
    assert [k for k in a if not _same(a[k], b[k])] == []
    assert any(k.endswith('/step') and float(v) == 4 for k, v in a.items())       # G: three loss steps + one path-length step
    for opt, nets in ((fresh.g_enc_optim, ('G', 'E_Tsr', 'E_W', 'E_W_Plus')), (fresh.d_optim, ('D',)),
                      (fresh.d_edit_optim, ('D_edit',))):     # the optimisers hold the live parameters
        live = {id(p) for k in nets for p in fresh.bare[k].parameters()}
        assert {id(p) for g in opt.param_groups for p in g['params']} == live
    assert (fresh.iter_idx, fresh.ds_count) == (tr.iter_idx, tr.ds_count) == (3, 1)
    assert torch.equal(torch.as_tensor(fresh.mean_path_length), torch.as_tensor(tr.mean_path_length))
    c1, c2 = copy.copy(tr), copy.copy(fresh)                 # ds_flags() advances ds_count: count on shallow copies
    assert [c1.ds_flags() for _ in range(4)] == [c2.ds_flags() for _ in range(4)] == \
        [(True, False), (True, True), (True, False), (True, False)]      # iter_idx 3 is a ds iteration; ds_count 1, 2, 3, 4
    assert tr.ds_count == 1


def test_reference_style_checkpoint_takes_the_iteration_from_the_file_name(trained, fresh, tmp_path):
    """A checkpoint without 'trainer', as the reference writes it: loads, iteration from the name ({iter:06d}.pt -> iter +
    1, train_3_encoder.py:438), ds_count and mean_path_length start at 0; as a dict it carries no iteration: ValueError."""
    tr = trained['tr']
    ck = tr.checkpoint()
    del ck['trainer']
    assert list(ck) == ['g', 'e_tsr', 'e_W', 'e_W_Plus', 'd', 'd_edit', 'g_ema', 'g_enc_optim', 'd_optim', 'd_edit_optim',
                        'co_mod', 'use_tanh', 'tsr_encode', 'sliced_layer']
    path = str(tmp_path / '000041.pt')
    torch.save(ck, path)
    fresh.load_checkpoint(path)
    assert (fresh.iter_idx, fresh.ds_count, fresh.mean_path_length) == (42, 0, 0)
    want, got = _tensors(tr), _tensors(fresh)
    assert [k for k in want if not torch.equal(want[k], got[k])] == []
    a, b = _optim_state(tr), _optim_state(fresh)
    assert [k for k in a if not _same(a[k], b[k])] == []
    with pytest.raises(ValueError, match='trainer'):
        fresh.load_checkpoint(ck)


def _spread(x, y):
    """Largest over the tensors of max|x - y| / max|x|, and the tensor it belongs to."""
    worst, where = 0.0, None
    for k, a in x.items():
        if not a.is_floating_point():
            continue
        scale = float(a.abs().max())
        d = float((a - y[k]).abs().max())
        if scale > 0 and d / scale > worst:
            worst, where = d / scale, k
    return worst, where


def test_resumed_trainer_continues_as_the_original(trained, fresh):
    tr = trained['tr']
    path = os.path.join(trained['ckpt_dir'], '000002.pt')
    first, second = _copy(tr), _copy(tr)
    resumed = fresh
    resumed.load_checkpoint(path)
    before = _tensors(first)
    before = {k: v.clone() for k, v in before.items()}
    flags = [_iterate(t, 3) for t in (first, second, resumed)]
    assert flags == [(True, False)] * 3 and first.iter_idx == second.iter_idx == resumed.iter_idx == 4
    a, b, r = _tensors(first), _tensors(second), _tensors(resumed)
    moved, _ = _spread(before, a)
    spread, where = _spread(a, b)
    got, got_where = _spread(a, r)
    print(f'CKPT iteration 4: update {moved:.3e}  run-to-run spread {spread:.3e} ({where})  resumed vs first {got:.3e} '
          f'({got_where})', flush=True)
    assert moved > 1e-4                                     # the iteration moved the parameters: the comparison is not empty
    bound = max(4.0 * spread, 1e-6)
    bad = []
    for k, t in a.items():
        if t.is_floating_point():
            d, scale = float((t - r[k]).abs().max()), float(t.abs().max())
            if d > bound * scale:
                bad.append((k, d / max(scale, 1e-300)))
        else:
            assert torch.equal(t, r[k]), k
    assert not bad, (bound, bad[:5])
    assert _same(first.ds_count, resumed.ds_count) and tr.iter_idx == 3      # the shared state was not touched
