"""CPU tests of the host logic of the visual evaluation: sheet layout and slot checks (op/canvas.py), the sample pickers,
path helpers and result names of Evaluation/visual_eval.py against selections recorded from the reference on fabricated
directories (tests/golden/visual_eval.json, tools/make_golden_visual_eval.py), the checkpoint's key list, and the launcher's
return codes."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import visual_eval_cases as vc
from nets import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(ROOT, 'tests', 'golden', 'visual_eval.json')) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------- op/canvas.py
def test_sheet_layout_arithmetic():
    from op.canvas import sheet_layout
    h, w, yx = sheet_layout(2, 3, 4, gap=1, margin=2)
    assert (h, w) == (2 * 2 + 2 * 4 + 1, 2 * 2 + 3 * 4 + 2 * 1)
    assert yx.tolist() == [[2, 2], [2, 7], [2, 12], [7, 2], [7, 7], [7, 12]]
    h, w, yx = sheet_layout(6, 5, 256, gap=8, margin=8)                   # the sample sheet of 6 sets
    assert (h, w) == (16 + 6 * 256 + 5 * 8, 16 + 5 * 256 + 4 * 8) and tuple(yx.shape) == (30, 2)
    assert yx[0].tolist() == [8, 8] and yx[-1].tolist() == [h - 8 - 256, w - 8 - 256]
    assert sheet_layout(1, 1, 7) == (7, 7, pytest.approx(np.zeros((1, 2))))
    # the tiles of a layout never overlap and lie inside the canvas: the slot check accepts them
    from op.canvas import check_slots
    for rows, cols, tile, gap, margin in ((3, 4, 5, 0, 0), (2, 2, 6, 3, 1), (1, 5, 4, 0, 2)):
        h, w, yx = sheet_layout(rows, cols, tile, gap, margin)
        s = check_slots(yx, rows * cols, tile, 1, h, w)
        assert s.dtype == np.int32 and s.shape == (rows * cols, 3) and not s[:, 0].any()
        with pytest.raises(ValueError):
            check_slots(yx, rows * cols, tile, 1, h - margin - 1, w)
        with pytest.raises(ValueError):
            check_slots(yx, rows * cols, tile, 1, h, w - margin - 1)
    for bad in ((0, 1, 4, 0, 0), (1, 0, 4, 0, 0), (1, 1, 0, 0, 0), (1, 1, 4, -1, 0), (1, 1, 4, 0, -1)):
        with pytest.raises(ValueError):
            sheet_layout(*bad)


def test_slots_bounds_and_overlap_are_refused():
    from op.canvas import check_slots, tiles_to_canvas
    ok = check_slots([(0, 0), (0, 4), (4, 0), (4, 4)], 4, 4, 1, 8, 8)       # touching is not overlapping
    assert ok.tolist() == [[0, 0, 0], [0, 0, 4], [0, 4, 0], [0, 4, 4]]
    assert check_slots([(1, 0, 0), (0, 0, 0)], 2, 4, 2, 4, 4).tolist() == [[1, 0, 0], [0, 0, 0]]   # same place, two canvases
    assert check_slots([], 0, 4, 1, 8, 8).shape == (0, 3)
    for slots, n in (([(0, 0), (3, 3)], 2), ([(0, 0), (0, 3)], 2), ([(0, 0), (3, 0)], 2), ([(2, 2), (2, 2)], 2),
                     ([(0, 0), (4, 4), (1, 5)], 3), ([(0, 6), (5, 0), (0, 0), (2, 3)], 4),                   # overlap
                     ([(5, 0)], 1), ([(0, 5)], 1), ([(-1, 0)], 1), ([(0, -1)], 1), ([(1, 0, 0)], 1), ([(-1, 0, 0)], 1),
                     ([(0, 0)], 2), ([(0, 0, 0, 0)], 1), ([(0.5, 0)], 1)):                                  # malformed
        with pytest.raises(ValueError):
            check_slots(slots, n, 4, 1, 8, 8)
    # the public call refuses the layout before it looks at the device: CPU tensors get the ValueError
    src, canvas = torch.zeros(2, 3, 4, 4), torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='overlap'):
        tiles_to_canvas(src, canvas, [(0, 0), (3, 3)], 4)
    with pytest.raises(ValueError, match='does not lie inside'):
        tiles_to_canvas(src, canvas, [(0, 0), (5, 0)], 4)
    with pytest.raises(ValueError, match='ratio'):
        tiles_to_canvas(torch.zeros(1, 3, 12, 12), canvas, [(0, 0)], 4)
    with pytest.raises(RuntimeError, match='CUDA tensor'):                 # a valid layout: no CPU path
        tiles_to_canvas(src, canvas, [(0, 0), (4, 4)], 4)
    assert not canvas.any()


def test_launcher_return_codes_are_host_logic():
    """fmgan_tiles_to_canvas refuses before any HIP call (the pointers are placeholders): EINVAL for non-positive sizes,
    null pointers and a ratio other than 1 / 2 / 4, OK for n == 0, EOVERFLOW beyond the 32-bit pixel and grid indices."""
    L = lib()
    fake = ctypes.c_void_p(0x1000)
    slots = ctypes.cast(fake, ctypes.POINTER(ctypes.c_int))
    OK, EINVAL, EOVER = 0, -1, -4

    def run(n=1, src=8, tile=8, nc=1, h=8, w=8, inp=fake, canvas=fake, sl=slots):
        return L.fmgan_tiles_to_canvas(inp, canvas, sl, n, src, tile, nc, h, w, 1.0, 127.5, None)
    for kw in (dict(n=-1), dict(src=0), dict(tile=0), dict(nc=0), dict(h=0), dict(w=0), dict(src=-8, tile=-8)):
        assert run(**kw) == EINVAL, kw
    for src, tile in ((12, 4), (32, 4), (9, 4), (4, 8), (10, 4)):
        assert run(src=src, tile=tile) == EINVAL, (src, tile)
    assert run(n=0) == OK and run(n=0, inp=None, canvas=None, sl=None) == OK
    assert run(n=0, src=12, tile=4) == EINVAL                               # the sizes are checked first
    for kw in (dict(inp=None), dict(canvas=None), dict(sl=None)):
        assert run(**kw) == EINVAL, kw
    assert run(src=46341, tile=46341) == EOVER                              # src^2 beyond 2^31
    assert run(n=1 << 30, src=4096, tile=1024) == EOVER                     # more blocks than grid.x holds
    assert run(nc=1 << 30, h=1 << 20, w=1 << 20) == EOVER                   # canvas bytes beyond 2^63


# ------------------------------------------------------------------------------------------------- pickers
def test_sample_pickers_pick_what_the_reference_picks(tmp_path, recorded):
    pytest.importorskip('PIL.Image')
    from Evaluation import visual_eval as ve
    assert ve.VAL_SET_LEN == vc.VAL_SET_LEN == 3 and ve.NUM_IMG_PER_ID == vc.NUM_IMG_PER_ID == 7
    paths = vc.write_real_stacks(tmp_path)
    vc.seed_pickers()
    real = ve.Get_Real_Img_Val_Sample(paths, vc.id_transform, vc.REAL_FACES, 'cpu')
    syn = ve.Get_Syn_Img_Val_Sample(vc.SynDataset(), vc.SYN_FACES, 'cpu')       # the generators run on, as recorded
    assert len(real) == vc.REAL_FACES * ve.VAL_SET_LEN and all(tuple(t.shape) == (1, 3, 8, 8) for t in real)
    assert vc.picked(real) == recorded['real_picks']
    assert len(syn) == 2 * ve.VAL_SET_LEN and all(tuple(t.shape) == (1, 3, 4, 4) for t in syn)
    assert vc.picked(syn) == recorded['syn_picks']
    # a set is (image, its render, another render of the same identity)
    for s in range(2):
        g, r, r2 = vc.picked(syn)[3 * s:3 * s + 3]
        assert r == -g - 1 and (-r2 - 1) // ve.NUM_IMG_PER_ID == g // ve.NUM_IMG_PER_ID


# ------------------------------------------------------------------------------------------------- paths and names
def test_path_helpers_match_the_reference(tmp_path, recorded):
    from Evaluation import visual_eval as ve
    single, video = tmp_path / 'single', tmp_path / 'video'
    single.mkdir(), video.mkdir()
    vc.touch(single, vc.SINGLE_FACTOR_FILES)
    vc.touch(video, vc.VIDEO_FILES)
    pairs = ve.Get_Img_Path_Single_Factor_Test(str(single))
    assert all(isinstance(p, tuple) for p in pairs)
    assert sorted(list(p) for p in pairs) == recorded['single_factor_pairs']      # os.listdir order is the file system's
    assert [list(p) for p in ve.Get_Img_Path_Video_Test(str(video))] == recorded['video_pairs']


def test_result_file_names_of_the_test_drivers(tmp_path, recorded, monkeypatch):
    Image = pytest.importorskip('PIL.Image')
    from Evaluation import visual_eval as ve
    frames = [np.full((8, 8, 3), 40 * t, np.uint8) for t in range(3)]
    calls = []

    def fake(kind):
        def run(a_path, b_path, model_modules, transform, device, **kwargs):
            calls.append((kind, os.path.basename(a_path), os.path.basename(b_path), kwargs))
            return frames
        return run
    monkeypatch.setattr(ve, 'Get_Single_Photo_Multi_Render_Result', fake('single'))
    monkeypatch.setattr(ve, 'Get_Multi_Photo_Multi_Render_Result', fake('multi'))
    single, video, save = tmp_path / 'single', tmp_path / 'video', tmp_path / 'save'
    single.mkdir(), video.mkdir(), save.mkdir()
    vc.touch(single, vc.SINGLE_FACTOR_FILES)
    vc.touch(video, vc.VIDEO_FILES)
    ve.Test_Single_Factor_Editing(str(single), str(save), 'modelA', None, None, 'cpu', chunk=4)
    assert sorted(os.listdir(save)) == recorded['single_factor_results']
    assert sorted(c[1:3] for c in calls) == sorted(tuple(p) for p in recorded['single_factor_pairs'])
    assert all(c[0] == 'single' and c[3] == {'chunk': 4} for c in calls)
    with Image.open(save / recorded['single_factor_results'][0]) as gif:
        assert gif.n_frames == 3 and gif.size == (8, 8)
    del calls[:]
    save2 = tmp_path / 'save2'
    save2.mkdir()
    ve.Test_Video_Reconstruction_Reanimation(str(video), str(save2), 'clip7', 'modelA', None, None, 'cpu')
    assert sorted(os.listdir(save2)) == sorted(recorded['video_results'])
    assert [c[:3] for c in calls] == [('single',) + tuple(recorded['video_pairs'][0]),
                                      ('multi',) + tuple(recorded['video_pairs'][1])]


# ------------------------------------------------------------------------------------------------- checkpoint keys
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(2))


def test_checkpoint_has_the_reference_keys_and_the_counters(recorded):
    """Trainer.checkpoint() on stand-in modules (no device needed): the reference's 14 names in its order, then 'trainer';
    d_edit / d_edit_optim None without a D_edit; default_args carries the four new fields."""
    import train_3_encoder as T3
    keys = recorded['checkpoint_keys']
    assert len(keys) == 14
    a = T3.default_args(grad_sync='flat')
    assert (a.val_sample_freq, a.model_save_freq, a.n_real_eval_faces, a.n_syn_eval_faces) == (1000, 10000, 2, 2)
    for with_edit in (False, True):
        nets = {k: _Tiny() for k in ('G', 'E_Tsr', 'E_W', 'E_W_Plus', 'D') + (('D_edit',) if with_edit else ())}
        tr = T3.Trainer(nets, a, device=torch.device('cpu'))
        tr.iter_idx, tr.ds_count, tr.mean_path_length = 7, 3, torch.tensor(0.25)
        ck = tr.checkpoint()
        assert list(ck) == keys + ['trainer']
        assert (ck['d_edit'] is None) == (ck['d_edit_optim'] is None) == (not with_edit)
        assert ck['co_mod'] is True and ck['use_tanh'] is a.use_tanh and ck['tsr_encode'] == a.tsr_encode
        assert ck['sliced_layer'] is None and list(ck['g']) == ['p'] and list(ck['g_ema']) == ['p']
        assert ck['trainer'] == {'iter_idx': 7, 'ds_count': 3, 'mean_path_length': torch.tensor(0.25)}
        assert len(ck['g_enc_optim']['param_groups'][0]['params']) == 4
    a.co_mod = False
    assert T3.Trainer(nets, a, device=torch.device('cpu')).checkpoint()['co_mod'] is False


def test_module_count_is_checked_before_anything_runs():
    from Evaluation import visual_eval as ve
    three = (None, None, None)
    x = torch.zeros(1, 3, 8, 8)
    for call in (lambda: ve.Get_Single_Eval_Result(x, [x, x], three),
                 lambda: ve.Get_Batch_Eval_Result([x, x, x], three),
                 lambda: ve.Batch_Eval_Sheet([x, x, x], three),
                 lambda: ve.Reconstruct_Frames(x, x, three),
                 lambda: ve.Reanimate_Frames(x, x, three)):
        with pytest.raises(ValueError, match='3-encoder scheme is the one this build provides'):
            call()


def test_checkpoint_file_round_trip_on_stand_in_modules(tmp_path):
    """save_checkpoint / load_checkpoint on CPU stand-ins (the GPU round trip is tests/test_checkpoint_gpu.py): the file
    name is that of the iteration just finished, parameters, Adam's moments and step counts and the counters come back,
    the optimisers hold the loaded modules' own parameters, and a file without 'trainer' takes the iteration from its name."""
    import train_3_encoder as T3

    def trainer(fill):
        nets = {k: _Tiny() for k in ('G', 'E_Tsr', 'E_W', 'E_W_Plus', 'D', 'D_edit')}
        for j, m in enumerate(nets.values()):
            m.p.data.fill_(fill + j)
        return T3.Trainer(nets, T3.default_args(grad_sync='flat'), device=torch.device('cpu'))
    tr = trainer(1.0)
    for steps, opt in ((3, tr.g_enc_optim), (2, tr.d_optim), (1, tr.d_edit_optim)):
        for s in range(steps):
            for g in opt.param_groups:
                for p in g['params']:
                    p.grad = torch.full_like(p, 0.5 + s)
            opt.step()
    tr.g_ema.p.data.fill_(9.0)
    tr.iter_idx, tr.ds_count, tr.mean_path_length = 5, 2, torch.tensor(0.75)
    path = tr.save_checkpoint(str(tmp_path / 'ckpt'))
    assert path == str(tmp_path / 'ckpt' / '000004.pt') and os.listdir(tmp_path / 'ckpt') == ['000004.pt']
    fresh = trainer(-3.0)
    wrapped = dict(fresh.nets)
    fresh.load_checkpoint(path)
    for k in tr.bare:
        assert torch.equal(fresh.bare[k].p, tr.bare[k].p) and fresh.nets[k] is wrapped[k]
    assert torch.equal(fresh.g_ema.p, tr.g_ema.p) and float(fresh.g_ema.p[0]) == 9.0
    for name, steps in (('g_enc_optim', 3), ('d_optim', 2), ('d_edit_optim', 1)):
        a, b = getattr(tr, name).state_dict(), getattr(fresh, name).state_dict()
        assert a['param_groups'] == b['param_groups'] and a['state'].keys() == b['state'].keys() and a['state']
        for idx in a['state']:
            assert float(b['state'][idx]['step']) == steps
            for field in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(a['state'][idx][field], b['state'][idx][field])
    assert {id(p) for g in fresh.g_enc_optim.param_groups for p in g['params']} == \
        {id(fresh.bare[k].p) for k in ('G', 'E_Tsr', 'E_W', 'E_W_Plus')}
    assert (fresh.iter_idx, fresh.ds_count, float(fresh.mean_path_length)) == (5, 2, 0.75)
    ck = tr.checkpoint()
    del ck['trainer']
    old = str(tmp_path / '000123.pt')
    torch.save(ck, old)
    other = trainer(0.0)
    other.load_checkpoint(old)
    assert (other.iter_idx, other.ds_count, other.mean_path_length) == (124, 0, 0)
    assert torch.equal(other.bare['D_edit'].p, tr.bare['D_edit'].p)
    with pytest.raises(ValueError, match='trainer'):
        other.load_checkpoint(ck)
