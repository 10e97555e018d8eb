"""CPU tests of the quantitative evaluation (Evaluation/quant_eval.py, op/eval_scores.py, csrc/eval_scores.hip): the
identity similarity against the reference's values, the loop logic of the two score functions on stand-in networks, the
host logic of the library's two entry points, and the register budget of the kernel."""
import ctypes

import numpy as np
import pytest
import torch

import codeobj
import quant_eval_cases as qc
import synth



def _face_model():
    from Util.arcface_pytorch.resnet_face_recognition import resnet_face18
    m = resnet_face18(use_se=False)
    m.load_state_dict(synth.state_dict('arcface', m.state_dict(), seed=9))
    return m.eval().requires_grad_(False)


# ------------------------------------------------------------------------------------------------ identity similarity
def test_identity_similarity_matches_reference_on_cpu(golden):
    """Compute_Face_Identity_Similarity on CPU tensors (the composite grey conversion), tensor and list forms, against the
    reference's per-sample values; the gate test_loss_networks.py holds the cosine form of the identity loss to on the CPU
    (rtol 20 * 2e-6, atol 1e-6)."""
    from Evaluation.quant_eval import Compute_Face_Identity_Similarity
    ref = golden('quant_eval')[qc.IDENTITY_CASE['name'] + '/cos']
    m = _face_model()
    target, outs = qc.identity_inputs()
    single = Compute_Face_Identity_Similarity(outs[0], target, m)
    listed = Compute_Face_Identity_Similarity(outs, target, m)
    assert torch.is_tensor(single) and tuple(single.shape) == (2,)
    assert isinstance(listed, list) and len(listed) == 2 and torch.equal(listed[0], single)
    for got, want in zip(listed, ref):
        np.testing.assert_allclose(got.numpy(), want, rtol=20 * 2e-6, atol=1e-6)
    assert float(ref[1].min()) > float(ref[0].max())          # the near-copy of the target is the more similar one


def test_face_input_composite_and_refusals_on_cpu(golden):
    """The composite equals Convert_Tensor_For_Face_Recognition_Loss / the reference's L1 line, face_input routes CPU
    tensors to it, and tensors that require grad are refused while grad mode is on."""
    from op import eval_scores as ES
    from Util.training_util import Convert_Tensor_For_Face_Recognition_Loss
    a = synth.tensor('face_id/a', (2, 3, 256, 256), dist='uniform')
    b = synth.tensor('face_id/b', (2, 3, 256, 256), dist='uniform')
    assert not ES.face_input_serves(a, b)
    ga, gb, l1 = ES.face_input(a, b, want_gray_b=True, want_l1=True)
    np.testing.assert_array_equal(ga.numpy(), golden('face_id')['converted'])
    assert torch.equal(gb, Convert_Tensor_For_Face_Recognition_Loss(b))
    assert torch.equal(l1, torch.mean(torch.abs(a - b), dim=(1, 2, 3)))
    assert ES.face_input(a)[1:] == (None, None)
    with pytest.raises(ValueError):
        ES.face_input(a, want_l1=True)
    with pytest.raises(RuntimeError, match='inference only'):
        ES.face_input(a.clone().requires_grad_(True))
    with torch.no_grad():
        assert torch.equal(ES.face_input(a.clone().requires_grad_(True))[0], ga)


# ------------------------------------------------------------------------------------------------ loop logic
def _code(p):
    return 0.5 * p.mean((2, 3), keepdim=True)


class _Standins:
    """Cheap replacements of the three forward functions, counting their calls.  image = photo-side code (0.5 * the
    photo's channel means) + 0.25 * render: depends on both inputs and has the render's size."""

    def __init__(self):
        self.calls = {'forward3': 0, 'encode': 0, 'reanimate': 0}

    def forward3(self, p, r, e_tsr, e_w, e_wp, g_ema, tsr_encode='Photo Image', sliced_layer=None, use_tanh=False):
        self.calls['forward3'] += 1
        out = _code(p) + 0.25 * r
        return torch.tanh(out) if use_tanh else out

    def encode(self, p, e_tsr, e_wp, tsr_encode='Photo Image'):
        self.calls['encode'] += 1
        return _code(p)

    def reanimate(self, code, r, e_tsr, e_w, g_ema, tsr_encode='Photo Image', sliced_layer=None, use_tanh=False,
                  noise=None, randomize_noise=True):
        self.calls['reanimate'] += 1
        out = code + 0.25 * r
        return torch.tanh(out) if use_tanh else out


def _face_diff(r, g):
    m = (r.mean(1, keepdim=True) > -1).float()
    return torch.mean(torch.square(r * m - g * m), dim=(1, 2, 3))


class _TinyFace(torch.nn.Module):
    """[N,1,h,w] grey image -> 6 features (mean-pooled to 2 x 3)."""

    def forward(self, x):
        return torch.nn.functional.adaptive_avg_pool2d(x, (2, 3)).reshape(x.shape[0], 6) + 0.1


def _standin_lpips(x, y):
    return ((x - y) ** 2).mean([1, 2, 3]).view(-1, 1, 1, 1)


@pytest.fixture
def patched(monkeypatch):
    from Evaluation import quant_eval as QE
    s = _Standins()
    monkeypatch.setattr(QE, 'Forward_Inference_3_Encoder', s.forward3)
    monkeypatch.setattr(QE, 'Encode_Photo', s.encode)
    monkeypatch.setattr(QE, 'Forward_Inference_Reanimate', s.reanimate)
    monkeypatch.setattr(QE, 'face_region_scores', _face_diff)      # the product's is a GPU kernel
    return QE, s


def _images(tag, n, size=16):
    return synth.tensor(f'qe_loop/{tag}', (n, 3, size, size), dist='uniform')


def _cos(face, a, b):
    from Util.training_util import Convert_Tensor_For_Face_Recognition_Loss as conv
    return torch.nn.functional.cosine_similarity(face(conv(a)), face(conv(b)))


@pytest.mark.parametrize('fuse', [True, False], ids=['fused', 'baseline'])
def test_recon_score_loop_on_cpu(patched, monkeypatch, fuse):
    QE, s = patched
    monkeypatch.setattr(QE, 'EVAL_FUSE', fuse)
    face = _TinyFace()
    loader = [(_images('p0', 3), _images('r0', 3)), (_images('p1', 2), _images('r1', 2)), (_images('p2', 1), _images('r2', 1))]
    scores = QE.Recon_Scores(loader, 'cpu', (None, None, None, None), (face, _standin_lpips), use_tanh=True)
    assert s.calls['forward3'] == 3 and s.calls['encode'] == 0
    want = {'cos': [], 'lpips': [], 'l1': []}
    for p, r in loader:
        g = torch.tanh(_code(p) + 0.25 * r)
        want['cos'].append(_cos(face, g, p))
        want['lpips'].append(_standin_lpips(g, p).reshape(-1))
        want['l1'].append((g - p).abs().mean((1, 2, 3)))
    for k in want:
        assert tuple(scores[k].shape) == (6,) and scores[k].dtype == torch.float32
        torch.testing.assert_close(scores[k], torch.cat(want[k]), rtol=1e-6, atol=1e-7)
    out = QE.Get_Recon_Score(loader, 'cpu', (None, None, None, None), (face, _standin_lpips), use_tanh=True)
    assert isinstance(out, tuple) and len(out) == 3 and all(isinstance(v, np.float64) for v in out)
    for v, k in zip(out, ('cos', 'lpips', 'l1')):
        assert v == np.mean(scores[k].double().numpy())         # float64 mean of the fp32 per-sample values


@pytest.mark.parametrize('fuse', [True, False], ids=['fused', 'baseline'])
def test_edit_score_loop_on_cpu(patched, monkeypatch, fuse):
    QE, s = patched
    monkeypatch.setattr(QE, 'EVAL_FUSE', fuse)
    face = _TinyFace()
    loader = [[_images('ep0', 2)] + [qc_render('er0', 2, i) for i in range(3)],
              [_images('ep1', 1)] + [qc_render('er1', 1, i) for i in range(3)]]
    scores = QE.Edit_Scores(loader, 'cpu', (None, None, None, None), (face, None, None), tsr_encode='Render Image')
    if fuse:       # the photo is encoded once per batch, every render runs the re-animation forward
        assert s.calls == {'forward3': 0, 'encode': 2, 'reanimate': 6}
    else:          # the reference's structure: all encoders per render
        assert s.calls == {'forward3': 6, 'encode': 0, 'reanimate': 0}
    cos, fd = [], []
    for batch in loader:                                         # render-major within a batch
        for r in batch[1:]:
            g = _code(batch[0]) + 0.25 * r
            cos.append(_cos(face, g, batch[0]))
            fd.append(_face_diff(r, g))
    assert tuple(scores['cos'].shape) == (9,) and tuple(scores['face_diff'].shape) == (9,)
    torch.testing.assert_close(scores['cos'], torch.cat(cos), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(scores['face_diff'], torch.cat(fd), rtol=1e-6, atol=1e-7)
    out = QE.Get_Edit_Score(loader, 'cpu', (None, None, None, None), (face, None, None), tsr_encode='Render Image')
    assert isinstance(out, tuple) and len(out) == 5 and out[1:4] == (None, None, None)
    assert out[0] == np.mean(scores['cos'].double().numpy()) and out[4] == np.mean(scores['face_diff'].double().numpy())


def qc_render(tag, n, index, size=16):
    """A small render in the manner of quant_eval_cases.render: exactly -1 outside a centred rectangle."""
    r = _images(tag + str(index), n, size)
    out = r.new_full(r.shape, -1.0)
    out[:, :, 3:13, 2 + index:12] = r[:, :, 3:13, 2 + index:12]
    return out


def test_score_functions_refuse_what_they_do_not_provide(patched, monkeypatch):
    QE, _ = patched
    face = _TinyFace()
    rec = [(_images('p0', 2), _images('r0', 2))]
    edit = [[_images('ep0', 2), qc_render('er0', 2, 0)]]
    with pytest.raises(ValueError, match='3-encoder'):
        QE.Get_Recon_Score(rec, 'cpu', (None, None, None), (face, _standin_lpips))
    with pytest.raises(ValueError, match='3-encoder'):
        QE.Get_Edit_Score(edit, 'cpu', (None, None, None), (face, None, None))
    with pytest.raises(ValueError, match='Inception'):
        QE.Get_Edit_Score(edit, 'cpu', (None,) * 4, (face, object(), None))
    with pytest.raises(ValueError, match='face_alignment'):
        QE.Get_Edit_Score(edit, 'cpu', (None,) * 4, (face, None, object()))
    # output and photo of different sizes (a 1024^2 generator on 256^2 photos): refused, not broadcast
    with pytest.raises(ValueError, match='pixel by pixel'):
        QE.Get_Recon_Score([(_images('p0', 2), _images('r8', 2, 8))], 'cpu', (None,) * 4, (face, _standin_lpips))
    # a render smaller than the output: the face difference is not broadcast either
    up = lambda *a, **k: torch.nn.functional.interpolate(a[1], scale_factor=2)      # noqa: E731  (a[1]: the render)
    for fuse in (True, False):
        monkeypatch.setattr(QE, 'EVAL_FUSE', fuse)
        monkeypatch.setattr(QE, 'Forward_Inference_3_Encoder', up)
        monkeypatch.setattr(QE, 'Forward_Inference_Reanimate', up)
        with pytest.raises(ValueError, match='pixel by pixel'):
            QE.Get_Edit_Score([[_images('ep0', 2), _images('er8', 2, 8)]], 'cpu', (None,) * 4, (face, None, None))


def test_eval_fuse_switch_follows_the_environment(monkeypatch):
    import importlib
    from Evaluation import quant_eval as QE
    try:
        monkeypatch.setenv('FMGAN_NO_EVAL_FUSE', '1')
        assert importlib.reload(QE).EVAL_FUSE is False
        monkeypatch.setenv('FMGAN_NO_EVAL_FUSE', '0')
        assert importlib.reload(QE).EVAL_FUSE is True
    finally:
        monkeypatch.delenv('FMGAN_NO_EVAL_FUSE')
        assert importlib.reload(QE).EVAL_FUSE is True          # the fused stage is the default


# ------------------------------------------------------------------------------------------------ host logic of the library
def test_face_input_host_logic():
    """fmgan_face_input_blocks / fmgan_face_input_f32: served shapes, partials per sample, argument checks, all before any
    HIP call (the pointers are placeholders)."""
    from op import _native
    L = _native.lib()
    blocks = L.fmgan_face_input_blocks
    assert blocks(64, 256, 256, 2) == 128 * 64 // 256              # one unit of 2 rows x 4 columns per lane
    assert blocks(2, 128, 128, 1) == 16 and blocks(1, 512, 512, 4) == 64 and blocks(8, 1024, 1024, 8) == 64
    assert blocks(3, 6, 10, 2) == 1 and blocks(1, 8, 24, 8) == 1
    for bad in ((64, 390, 390, 3), (64, 256, 256, 3), (64, 255, 256, 2), (64, 256, 254, 4), (0, 256, 256, 2),
                (-1, 256, 256, 2), (64, 0, 256, 2), (64, 256, -4, 2), (64, 256, 256, 0), (64, 256, 256, 16),
                (1, 65536, 65536, 1), (1 << 30, 256, 256, 1)):
        assert blocks(*bad) == 0, bad
    fake = ctypes.c_void_p(0x1000)
    EINVAL, EUNSUP, EOVER = -1, -2, -4
    run = L.fmgan_face_input_f32
    shape = (2, 256, 256, 2, None)
    assert run(None, fake, fake, fake, fake, *shape) == EINVAL                 # no first image
    assert run(fake, fake, None, None, None, *shape) == EINVAL                 # no output at all
    assert run(fake, None, fake, fake, None, *shape) == EINVAL                 # gray_b without b
    assert run(fake, None, fake, None, fake, *shape) == EINVAL                 # l1_partial without b
    assert run(fake, None, None, None, fake, *shape) == EINVAL
    assert run(fake, fake, fake, fake, fake, 0, 256, 256, 2, None) == EINVAL
    assert run(fake, fake, fake, fake, fake, 2, 390, 390, 3, None) == EUNSUP
    assert run(fake, fake, fake, fake, fake, 2, 255, 256, 2, None) == EUNSUP
    assert run(fake, fake, fake, fake, fake, 1, 65536, 65536, 1, None) == EOVER
    assert run(fake, fake, fake, fake, fake, 1 << 30, 256, 256, 1, None) == EOVER


# ------------------------------------------------------------------------------------------------ register budget
@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    """The notes of the face-input kernels; codeobj.kernel_notes builds the library first if a fresh checkout has none."""
    notes = codeobj.kernel_notes(tmp_path_factory.mktemp('codeobj'))
    return {name: k for name, k in notes.items() if 'face_input_f32' in name}


def test_face_input_kernel_budget(kernels):
    """Every instantiation (k in 1 / 2 / 4 / 8, 16-byte and scalar form, one image and a pair) is present, without spills or
    scratch, in at most 128 registers: blocks are 256 lanes (one wave per SIMD), a lane keeps at most 24 16-byte loads in
    flight (96 registers) beside its window sums and addresses, and 128 registers let four such blocks share a CU."""
    assert len(kernels) == 16, sorted(kernels)
    for k in (1, 2, 4, 8):
        for vec in (0, 1):
            for pair in (0, 1):
                assert sum(f'ILi{k}ELb{vec}ELb{pair}E' in n for n in kernels) == 1, (k, vec, pair)
    for name, k in sorted(kernels.items()):
        print(name, k)
        assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0, (name, k)
        assert k['vgpr'] <= 128, (name, k)
