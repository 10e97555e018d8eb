"""CPU tests of the FID (Evaluation/fid.py, calc_inception.py, inception.py, op/fid_stats.py, op/inception_input.py):
calc_fid and the sampling loop against the reference's values, the running statistics against numpy, the Inception
topology, the FID slot of Get_Edit_Score, the host logic of the new entry points and the resources of the new kernels."""
import numpy as np
import pytest
import torch

import codeobj
import fid_cases as fc
from nets import lib


# ------------------------------------------------------------------------------------------------ calc_fid
@pytest.mark.parametrize('case', fc.CALC_CASES, ids=[c[0] for c in fc.CALC_CASES])
def test_calc_fid_matches_reference(golden, case):
    """The eigenvalue form of tr sqrt(S1 S2) against the reference's scipy.linalg.sqrtm form, on the reference's inputs
    (fp32 np.mean, float64 np.cov), within 10 x the reference's own spread (tests/fid_cases.py); numpy and tensor
    arguments give the same float."""
    from Evaluation.fid import calc_fid
    name, d, n1, n2 = case
    g = golden('fid')
    (ma, ca), (mb, cb) = fc.moments(fc.features(name, 'a', n1, d)), fc.moments(fc.features(name, 'b', n2, d))
    got = calc_fid(ma, ca, mb, cb)
    want, tol = float(g[name + '/fid']), fc.tolerance(g, name)
    print(f'{name}: fid {got!r} reference {want!r} |diff| {abs(got - want):.3e} tolerance {tol:.3e}')
    assert isinstance(got, float) and tol > 0
    assert abs(got - want) <= tol
    assert calc_fid(torch.from_numpy(ma), torch.from_numpy(ca), torch.from_numpy(mb), torch.from_numpy(cb)) == got
    assert abs(calc_fid(ma, ca, ma, ca)) <= tol          # the distance of a distribution from itself


# ------------------------------------------------------------------------------------------------ running statistics
def _accumulate(feat, batch, device='cpu', **kw):
    from op.fid_stats import Feature_Statistics
    stats = Feature_Statistics(feat.shape[1], device, **kw)
    for i in range(0, feat.shape[0], batch):
        stats.update(torch.from_numpy(feat[i:i + batch]))
    return stats


def _check_against_numpy(stats, feat):
    """mean / cov of the state against np.mean(float64) / np.cov of all the features, within fid_cases.moment_bounds."""
    f64 = feat.astype(np.float64)
    mean, cov = (t.cpu().numpy() for t in stats.finish())
    mean_bound, cov_bound = fc.moment_bounds(f64, stats.shift.cpu().numpy())
    want_mean, want_cov = np.mean(f64, 0), np.cov(f64, rowvar=False)
    print('max |mean diff| / bound', float((np.abs(mean - want_mean) / mean_bound).max()),
          'max |cov diff| / bound', float((np.abs(cov - want_cov) / cov_bound).max()),
          'relative to max |cov|', float(np.abs(cov - want_cov).max() / np.abs(want_cov).max()))
    assert stats.count == feat.shape[0] and mean.dtype == np.float64 and cov.dtype == np.float64
    assert (np.abs(mean - want_mean) <= mean_bound).all()
    assert (np.abs(cov - want_cov) <= cov_bound).all()
    assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize('d', [64, 52], ids=['d64', 'd52'])
def test_feature_statistics_composite_matches_numpy(d):
    """Batches of 37 (the last one short) against numpy on the concatenation; default shift and a given one."""
    feat = fc.features('stats', 'a', 200, d)
    stats = _accumulate(feat, 37)
    assert torch.equal(stats.shift, torch.from_numpy(feat[:37]).double().mean(0))
    _check_against_numpy(stats, feat)
    _check_against_numpy(_accumulate(feat, 37, shift=np.full(d, 0.25)), feat)
    with pytest.raises(ValueError):
        stats.update(torch.zeros(3, d + 1))
    with pytest.raises(ValueError, match='two'):
        _accumulate(feat[:1], 37).finish()


def test_feature_statistics_merge():
    """Two halves accumulated with different shifts (each its first batch's mean), merged: the statistics of the whole,
    within the same bounds; merging into an empty state adopts the other's."""
    from op.fid_stats import Feature_Statistics
    feat = fc.features('stats', 'b', 207, 64)
    a, b = _accumulate(feat[:90], 37), _accumulate(feat[90:], 37)
    assert not torch.equal(a.shift, b.shift)
    shift = a.shift.clone()
    a.merge(b)
    assert a.count == 207 and torch.equal(a.shift, shift)
    _check_against_numpy(a, feat)
    empty = Feature_Statistics(64, 'cpu').merge(_accumulate(feat, 37))
    _check_against_numpy(empty, feat)


# ------------------------------------------------------------------------------------------------ the sampling loop
def test_sample_statistics_and_extract_match_reference(golden):
    """The reference's extract_feature_from_samples -> np.cov -> calc_fid on the toy generator and the stand-in
    inception, with fixed latents and the uneven split 32 + 38, against Sample_Statistics -> finish -> calc_fid."""
    from Evaluation import fid as FID
    c = fc.SAMPLE_BY_NAME['toy']
    g = golden('fid')
    assert FID.batch_split(c['n_sample'], c['batch']) == [32, 38]
    gen, inc, real = fc.ToyGenerator(), fc.StandinInception(), fc.real_stats()
    stats = FID.Sample_Statistics(gen, inc, 1, None, c['batch'], c['n_sample'], 'cpu', sampler=fc.sampler(c))
    assert stats.count == 70 and stats.dim == fc.FEATURES
    got = FID.calc_fid(*stats.finish(), real['mean'], real['cov'])
    want, tol = float(g['sample_toy/fid']), fc.tolerance(g, 'sample_toy')
    print(f'toy: fid {got!r} reference {want!r} |diff| {abs(got - want):.3e} tolerance {tol:.3e}')
    assert abs(got - want) <= tol
    feat = FID.extract_feature_from_samples(gen, inc, 1, None, c['batch'], c['n_sample'], 'cpu', sampler=fc.sampler(c))
    assert tuple(feat.shape) == (70, fc.FEATURES) and feat.device.type == 'cpu'
    _check_against_numpy(stats, feat.numpy())
    with pytest.raises(ValueError, match='no batch'):
        FID.batch_split(5, 8)


def test_get_model_fid_score_arguments(tmp_path):
    """real_stats as a dict and as a pickle path give one value; without it the error names the reference's file."""
    import pickle
    from Evaluation import fid as FID
    gen, inc, real = fc.ToyGenerator(), fc.StandinInception(), fc.real_stats()
    torch.manual_seed(1)
    a = FID.Get_Model_FID_Score(gen, device='cpu', batch_size=16, num_sample=40, inception=inc, real_stats=real)
    path = tmp_path / 'stats.pkl'
    path.write_bytes(pickle.dumps(real))
    torch.manual_seed(1)
    b = FID.Get_Model_FID_Score(gen, device='cpu', batch_size=16, num_sample=40, inception=inc, real_stats=str(path),
                                gpu_device_ids=[0])
    assert isinstance(a, float) and a == b and a > 0
    with pytest.raises(ValueError, match='inception_ffhq_embed'):
        FID.Get_Model_FID_Score(gen, device='cpu', inception=inc)


def test_fid_fuse_switch_follows_the_environment(monkeypatch):
    import importlib
    from Evaluation import fid as FID
    try:
        monkeypatch.setenv('FMGAN_NO_FID_FUSE', '1')
        assert importlib.reload(FID).FID_FUSE is False
    finally:
        monkeypatch.delenv('FMGAN_NO_FID_FUSE')
        assert importlib.reload(FID).FID_FUSE is True


# ------------------------------------------------------------------------------------------------ the network
@pytest.fixture(scope='module')
def inception_run():
    """One InceptionV3 with all four output blocks in float64 on the CPU at B = 1: (module, image, folded outputs,
    module-by-module outputs, {layer name: output shape} recorded during the module-by-module forward)."""
    from Evaluation.inception import InceptionV3
    torch.manual_seed(0)
    m = InceptionV3([0, 1, 2, 3]).double().eval()
    shapes, hooks = {}, []
    for name, child in m.named_children():
        hooks.append(child.register_forward_hook(lambda mod, i, o, name=name: shapes.__setitem__(name, tuple(o.shape))))
    x = torch.rand(1, 3, 64, 64, dtype=torch.float64)
    with torch.no_grad():
        plain = m.forward_modules(x)
        for h in hooks:
            h.remove()
        folded = m(x)
    return m, x, folded, plain, shapes


def test_inception_topology(inception_run):
    m, x, folded, plain, shapes = inception_run
    assert [tuple(t.shape) for t in plain] == [(1, 64, 73, 73), (1, 192, 35, 35), (1, 768, 17, 17), (1, 2048, 1, 1)]
    want = {'Conv2d_1a_3x3': (32, 149), 'Conv2d_2a_3x3': (32, 147), 'Conv2d_2b_3x3': (64, 147), 'Conv2d_3b_1x1': (80, 73),
            'Conv2d_4a_3x3': (192, 71), 'Mixed_5b': (256, 35), 'Mixed_5c': (288, 35), 'Mixed_5d': (288, 35),
            'Mixed_6a': (768, 17), 'Mixed_6b': (768, 17), 'Mixed_6c': (768, 17), 'Mixed_6d': (768, 17),
            'Mixed_6e': (768, 17), 'Mixed_7a': (1280, 8), 'Mixed_7b': (2048, 8), 'Mixed_7c': (2048, 8)}
    assert shapes == {k: (1, c, s, s) for k, (c, s) in want.items()}
    assert tuple(m.fc.weight.shape) == (1008, 2048)
    assert not any(p.requires_grad for p in m.parameters())
    convs = [k for k in m.state_dict() if k.endswith('.conv.weight')]
    assert len(convs) == 94 and 'Conv2d_1a_3x3.conv.weight' in convs
    assert 'Mixed_5b.branch1x1.bn.running_var' in m.state_dict() and 'Mixed_7c.branch3x3dbl_3b.bn.bias' in m.state_dict()
    assert m.Mixed_7b.pool == 'avg' and m.Mixed_7c.pool == 'max'
    assert all(mod.eps == 0.001 for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))


def test_inception_folded_forward_matches_modules(inception_run):
    """BatchNorm folded into the convolutions, channels_last: against the module-by-module form in float64 (after moving
    the BatchNorm statistics off their initial 0 / 1, so that the fold has something to fold)."""
    from Evaluation.inception import InceptionV3
    m, x, folded, plain, _ = inception_run
    for a, b in zip(folded, plain):
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(5)
    for k, v in sd.items():
        if k.endswith('running_mean') or k.endswith('bn.bias'):
            v.copy_(0.1 * torch.randn(v.shape, generator=gen, dtype=v.dtype))
        elif k.endswith('running_var') or k.endswith('bn.weight'):
            v.copy_(0.5 + torch.rand(v.shape, generator=gen, dtype=v.dtype))
    sd = {k: v.float().double() if v.is_floating_point() else v for k, v in sd.items()}    # the module is built in fp32
    other = InceptionV3([3], weights=sd).double().eval()          # the state_dict round trip, through `weights=`
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    with torch.no_grad():
        a, b = other(x)[0], other.forward_modules(x)[0]
        first = other.Conv2d_1a_3x3.folded()[0]
        assert other.Conv2d_1a_3x3.folded()[0] is first               # folded once per weight version
        other.load_weights(m.state_dict())
        assert other.Conv2d_1a_3x3.folded()[0] is not first
        again = other(x)[0]
    assert tuple(a.shape) == (1, 2048, 1, 1) and float(b.abs().max()) > 0
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    assert float((again - plain[3]).abs().max()) <= 1e-12 * float(plain[3].abs().max())
    with pytest.raises(RuntimeError):                                  # strict about everything else
        other.load_weights({k: v for k, v in sd.items() if k != 'fc.bias'})


def test_patched_inception_and_input_stage_on_cpu():
    """load_patched_inception_v3 as the reference builds it; the input stage routes CPU tensors to the composite, which
    is F.interpolate and 2x - 1 in channels_last, and refuses autograd."""
    import torch.nn.functional as F
    from Evaluation.calc_inception import load_patched_inception_v3
    from op import inception_input as II
    m = load_patched_inception_v3()
    assert m.output_blocks == [3] and m.normalize_input is False and m.resize_input is True
    x = torch.rand(2, 3, 32, 32)
    assert not II.inception_input_serves(x)
    y = II.inception_input(x)
    assert tuple(y.shape) == (2, 3, 299, 299) and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, 2 * F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False) - 1)
    assert torch.equal(II.inception_input(x, normalize_input=False, resize_input=False), x)
    with pytest.raises(RuntimeError, match='inference only'):
        II.inception_input(x.clone().requires_grad_(True))


# ------------------------------------------------------------------------------------------------ Get_Edit_Score
def test_get_edit_score_fills_the_fid_slot(monkeypatch):
    """With an inception model and fid_stats the FID slot holds calc_fid of the statistics of every output's features
    against fid_stats; the outputs of a batch go through the model in one call; without fid_stats: ValueError."""
    import test_quant_eval as tq
    from Evaluation import quant_eval as QE
    from Evaluation.fid import calc_fid
    s = tq._Standins()
    monkeypatch.setattr(QE, 'Forward_Inference_3_Encoder', s.forward3)
    monkeypatch.setattr(QE, 'Encode_Photo', s.encode)
    monkeypatch.setattr(QE, 'Forward_Inference_Reanimate', s.reanimate)
    monkeypatch.setattr(QE, 'face_region_scores', tq._face_diff)
    face, real = tq._TinyFace(), fc.real_stats()
    calls = []

    class Counting(fc.StandinInception):
        def forward(self, img):
            calls.append(img.shape[0])
            return super().forward(img)
    inc = Counting()
    loader = [[tq._images('ep0', 2)] + [tq.qc_render('er0', 2, i) for i in range(3)],
              [tq._images('ep1', 1)] + [tq.qc_render('er1', 1, i) for i in range(3)]]
    feats = []
    for batch in loader:                                          # render-major within a batch, one call per batch
        outputs = torch.cat([tq._code(batch[0]) + 0.25 * r for r in batch[1:]])
        feats.append(fc.StandinInception()(outputs)[0].flatten(1))
    feats = torch.cat(feats).numpy()
    want = calc_fid(np.mean(feats.astype(np.float64), 0), np.cov(feats, rowvar=False), real['mean'], real['cov'])
    for fuse in (True, False):
        monkeypatch.setattr(QE, 'EVAL_FUSE', fuse)
        del calls[:]
        out = QE.Get_Edit_Score(loader, 'cpu', (None,) * 4, (face, inc, None), tsr_encode='Render Image', fid_stats=real)
        assert calls == [6, 3]
        assert len(out) == 5 and out[2:4] == (None, None) and isinstance(out[1], float)
        assert abs(out[1] - want) <= 1e-9 * abs(want)
    with pytest.raises(ValueError, match='Inception'):
        QE.Get_Edit_Score(loader, 'cpu', (None,) * 4, (face, inc, None), tsr_encode='Render Image')
    assert QE.Get_Edit_Score(loader, 'cpu', (None,) * 4, (face, None, None), tsr_encode='Render Image')[1] is None


# ------------------------------------------------------------------------------------------------ host logic, budgets
def test_entry_points_host_logic():
    """Plans and argument checks of the new entry points, all before any HIP call (pointers are placeholders or null)."""
    import ctypes
    L = lib()
    EINVAL, EUNSUP, EOVER = -1, -2, -4
    fake = ctypes.c_void_p(0x1000)
    assert L.fmgan_fid_stats_select(100, 2048) == 1 and L.fmgan_fid_stats_select(1, 16) == 1
    assert L.fmgan_fid_stats_select(4, 24) == EUNSUP and L.fmgan_fid_stats_select(4, 2047) == EUNSUP
    assert L.fmgan_fid_stats_select(0, 16) == EINVAL and L.fmgan_fid_stats_select(4, 0) == EINVAL
    assert L.fmgan_fid_stats_select(4, (1 << 21) + 16) == EOVER
    assert L.fmgan_fid_stats_update_f32(fake, fake, fake, fake, 4, 24, None) == EUNSUP
    assert L.fmgan_fid_stats_update_f32(None, fake, fake, fake, 4, 16, None) == EINVAL
    assert L.fmgan_fid_stats_finish_f64(fake, fake, fake, 1, fake, fake, 16, None) == EINVAL
    assert L.fmgan_fid_stats_finish_f64(fake, fake, None, 5, fake, fake, 16, None) == EINVAL
    for s, want in ((256, 1), (512, 1), (1024, 1), (299, 2), (300, EUNSUP), (128, EUNSUP)):
        assert L.fmgan_inception_input_select(2, s, s) == want, s
    assert L.fmgan_inception_input_select(2, 256, 512) == EUNSUP and L.fmgan_inception_input_select(0, 256, 256) == EINVAL
    assert L.fmgan_inception_input_select(1 << 24, 256, 256) == EOVER
    assert L.fmgan_inception_input_f32(fake, fake, 2, 300, 300, 1, None) == EUNSUP
    assert L.fmgan_inception_input_f32(None, fake, 2, 256, 256, 1, None) == EINVAL


def test_new_kernels_are_built_without_spills_or_scratch(tmp_path):
    """csrc/fid_stats.hip and csrc/inception_input.hip in the built library: the update and finish kernels and the two
    forms of the input stage, no spills, no scratch (the update kernel holds 16 accumulator doubles per lane)."""
    notes = codeobj.kernel_notes(tmp_path)
    mine = {n: k for n, k in notes.items() if 'fid_stats' in n or 'inception_input' in n}
    assert sum('fid_stats_update_f32' in n for n in mine) == 1 and sum('fid_stats_finish_f64' in n for n in mine) == 1
    assert sum('inception_input_f32' in n for n in mine) == 2 and len(mine) == 4, sorted(mine)
    for name, k in sorted(mine.items()):
        print(name, k)
        assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0, (name, k)
        # 168 registers keep three waves on a SIMD (512 / 3); the update's grid at D = 2048 supplies two (528 blocks of four
        # waves on 1024 SIMDs), and it holds 16 accumulator doubles and the 20 loads of four steps in flight
        assert k['vgpr'] <= 168 and k['lds'] == 0, (name, k)
