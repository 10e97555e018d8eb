"""GPU tests of the drivers of Evaluation/visual_eval.py: the sample grid and the video reconstruction against the
reference's own runs (tests/golden/visual_eval.npz, tools/make_golden_visual_eval.py: full-width seeded networks), the
sheet and the triptychs against the list drivers, chunking, and the GIF driver.

Bit comparisons between two runs use fixed-matrix encoders on deterministic kernels (tests/test_reanimate.py:
_FixedEncoder) and narrow Generators: the library convolutions of the real encoders are not bit-reproducible run to run.
Chunking: the project's existing chunk test (test_reanimate_frames_chunked_golden) does not demand bit equality between
chunk sizes for this path (tile selection and the encoders' kernels depend on the batch); its criterion is applied
instead — every chunk size passes the end-to-end gate against the fixture, frame by frame."""
import numpy as np
import pytest
import torch

import synth
import visual_eval_cases as vc
from gpumem import dev
from nets import PinNoise, encoders, load
from parity import img_close
from test_canvas_gpu import _reduced
from test_reanimate import _FixedEncoder, _narrow_g

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def nets256():
    import stylegan2
    return encoders(14) + (PinNoise(load(stylegan2.Generator(256, 512, 8), 'generator', 4)),)


def _fixed_modules(size, width=32):
    """Deterministic encoders and a narrow Generator(size) of `width` channels throughout, noise pinned."""
    import stylegan2
    n_latent = int(np.log2(size)) * 2 - 2
    G = load(stylegan2.Generator(size, 512, 1, generator_net_shape=[width] * n_latent), 'generator', 4)
    return (_FixedEncoder('tsr', (width, 4, 4), 0.5, 0.0).to(dev()), _FixedEncoder('w', (512,), 0.5, 0.0).to(dev()),
            _FixedEncoder('wp', (n_latent, 512), 0.2, 1.0).to(dev()), PinNoise(G))


def _check_u8(images, g, c, output_at):
    """The strided uint8 images against the fixture's: inputs equal, outputs under the rule of
    visual_eval_cases.u8_rule_violations with the fixture's float values."""
    s, n = c['stride'], c['name']
    got = np.stack(images)[:, ::s, ::s]
    ref = g[n + '/u8']
    assert got.shape == ref.shape and got.dtype == np.uint8
    outs = [i for i in range(len(images)) if output_at(i)]
    others = [i for i in range(len(images)) if not output_at(i)]
    np.testing.assert_array_equal(got[others], ref[others])
    assert len(outs) == g[n + '/sub'].shape[0]
    changed = int((got[outs] != ref[outs]).sum())
    bad = vc.u8_rule_violations(got[outs], ref[outs], g[n + '/sub'])
    print(f'U8 {n}: {changed} of {got[outs].size} entries differ from the reference, {bad} break the rule', flush=True)
    assert bad == 0


def _gate(floats, g, c):
    img_close(floats.detach().float().cpu().numpy(), g[c['name'] + '/sub'], g[c['name'] + '/stats'], c['stride'],
              g[c['name'] + '/sub64'], vc.REL)


# ------------------------------------------------------------------------------------------------- reference parity
def test_batch_eval_result_golden(golden, nets256):
    from Evaluation.visual_eval import Get_Batch_Eval_Result, Get_Single_Eval_Result, Reanimate_Frames
    c, g = vc.BATCH, golden('visual_eval')
    imgs = [t.to(dev()) for t in vc.batch_inputs(c)]
    kw = dict(vc.fwd_kwargs(c), randomize_noise=False)
    images = Get_Batch_Eval_Result(imgs, nets256, **kw)
    assert len(images) == 5 * c['sets'] and all(i.dtype == np.uint8 and i.shape == (256, 256, 3) for i in images)
    _check_u8(images, g, c, lambda i: i % 5 in (2, 4))
    single = Get_Single_Eval_Result(imgs[0], imgs[1:3], nets256, **kw)
    assert len(single) == 5
    for a, b in zip(single[:2] + single[3:4], images[:2] + images[3:4]):          # photo and renders: exact
        np.testing.assert_array_equal(a, b)
    # the float outputs behind the pictures (the same path: photo encoded once, the renders in one forward)
    floats = [Reanimate_Frames(imgs[3 * s], torch.cat(imgs[3 * s + 1:3 * s + 3]), nets256, return_float=True, **kw)[1]
              for s in range(c['sets'])]
    _gate(torch.cat(floats, 0), g, c)


@pytest.mark.parametrize('chunk', [1, 2, 8])
def test_reconstruct_frames_golden_at_every_chunk_size(chunk, golden, nets256):
    """Three photo / render pairs in chunks of 1, 2 + 1 and 3: every frame, in order, passes the gate against the
    reference's loop (the criterion of test_reanimate_frames_chunked_golden), and the uint8 frames keep the uint8 rule."""
    from Evaluation.visual_eval import Reconstruct_Frames, tensor2im_batch
    c, g = vc.VIDEO, golden('visual_eval')
    p, r = vc.video_inputs(c)
    p = [t.to(dev()) for t in p]
    images, floats = Reconstruct_Frames(p, r, nets256, chunk=chunk, return_float=True, **vc.fwd_kwargs(c))
    assert len(images) == 3 and tuple(floats.shape) == (3, 3, 256, 256)
    _gate(floats, g, c)
    scale = float(np.abs(g[c['name'] + '/sub']).max())
    for t in range(3):
        a = floats[t].cpu().numpy()[..., ::c['stride'], ::c['stride']]
        np.testing.assert_allclose(a, g[c['name'] + '/sub'][t], atol=vc.REL * scale, rtol=vc.REL)
    np.testing.assert_array_equal(np.stack(images), tensor2im_batch(floats).cpu().numpy())
    _check_u8(images, g, c, lambda i: True)


# ------------------------------------------------------------------------------------------------- the sheet
def _sheet_inputs(tag, sets):
    return [t.to(dev()) for t in vc.batch_inputs(dict(vc.BATCH, name=tag, sets=sets))]


def test_batch_eval_sheet_equals_the_list_at_256():
    """tile = 256 with a Generator(256): every tile is the corresponding array of Get_Batch_Eval_Result, everything else
    is the background; three launches for the whole sheet."""
    from Evaluation.visual_eval import Batch_Eval_Sheet, Get_Batch_Eval_Result
    from launches import observed
    from op.canvas import sheet_layout
    mods = _fixed_modules(256)
    imgs = _sheet_inputs('sheet256', 3)
    images = Get_Batch_Eval_Result(imgs, mods, randomize_noise=False)
    with observed() as rec:
        sheet = Batch_Eval_Sheet(imgs, mods, tile=256, gap=8, margin=8, background=200, randomize_noise=False)
    assert rec.count('tiles_to_canvas') == 3
    h, w, yx = sheet_layout(3, 5, 256, 8, 8)
    assert sheet.dtype == torch.uint8 and tuple(sheet.shape) == (h, w, 3) and sheet.device == dev()
    host = sheet.cpu().numpy()
    rest = np.ones((h, w), bool)
    assert len(images) == 15
    for k, (y0, x0) in enumerate(yx):
        np.testing.assert_array_equal(host[y0:y0 + 256, x0:x0 + 256], images[k], err_msg=f'tile {k}')
        rest[y0:y0 + 256, x0:x0 + 256] = False
    assert (host[rest] == 200).all() and rest.sum() == h * w - 15 * 256 * 256
    assert len({images[k].tobytes() for k in range(15)}) == 15                    # fifteen different pictures


def test_batch_eval_sheet_reduces_1024_outputs_by_four():
    """A narrow Generator(1024) beside 256^2 inputs: the outputs' tiles are the kernel's reduction by 4 (the formula of
    tests/test_canvas_gpu.py), the inputs' tiles the pixels themselves."""
    from Evaluation.visual_eval import Batch_Eval_Sheet, Reanimate_Frames, tensor2im_batch
    from op.canvas import sheet_layout
    mods = _fixed_modules(1024)
    imgs = _sheet_inputs('sheet1024', 1)
    sheet = Batch_Eval_Sheet(imgs, mods, tile=256, gap=4, margin=2, randomize_noise=False)
    h, w, yx = sheet_layout(1, 5, 256, 4, 2)
    assert tuple(sheet.shape) == (h, w, 3)
    _, floats = Reanimate_Frames(imgs[0], torch.cat(imgs[1:3]), mods, return_float=True, randomize_noise=False)
    assert tuple(floats.shape) == (2, 3, 1024, 1024)
    outs = tensor2im_batch(_reduced(floats, 4))
    tiles = [tensor2im_batch(imgs[0])[0], tensor2im_batch(imgs[1])[0], outs[0], tensor2im_batch(imgs[2])[0], outs[1]]
    for k, (y0, x0) in enumerate(yx):
        assert torch.equal(sheet[y0:y0 + 256, x0:x0 + 256], tiles[k]), f'tile {k}'
    assert bool((sheet[:2] == 255).all()) and bool((sheet[:, 258:262] == 255).all())


def test_sheet_and_frames_refuse_other_ratios_and_module_counts():
    from Evaluation import visual_eval as ve
    G = _narrow_g()                                                      # 64^2 outputs
    mods = (_FixedEncoder('tsr', (16, 4, 4), 0.5, 0.0).to(dev()), _FixedEncoder('w', (512,), 0.5, 0.0).to(dev()),
            _FixedEncoder('wp', (G.n_latent, 512), 0.2, 1.0).to(dev()), PinNoise(G))
    imgs = _sheet_inputs('refuse', 1)
    with pytest.raises(ValueError, match='ratio must be 1, 2 or 4'):
        ve.Batch_Eval_Sheet(imgs, mods, tile=256, randomize_noise=False)
    with pytest.raises(ValueError, match='ratio must be 1, 2 or 4'):
        ve.Reconstruct_Frames(imgs[:1], imgs[1:2], mods, triptych=True, tile=48)
    sheet = ve.Batch_Eval_Sheet(imgs, mods, tile=64, gap=0, margin=0, randomize_noise=False)      # 256 -> 64: by four
    assert tuple(sheet.shape) == (64, 320, 3)
    three = mods[:2] + mods[3:]
    for call in (lambda: ve.Batch_Eval_Sheet(imgs, three), lambda: ve.Get_Batch_Eval_Result(imgs, three),
                 lambda: ve.Reconstruct_Frames(imgs[:1], imgs[1:2], three),
                 lambda: ve.Get_Multi_Photo_Multi_Render_Result('a.gif', 'b.gif', three, None, dev())):
        with pytest.raises(ValueError, match='3-encoder scheme is the one this build provides'):
            call()


# ------------------------------------------------------------------------------------------------- frames
def test_reconstruct_frames_lengths_and_triptych():
    """Unequal lengths stop at the shorter; a triptych is [photo | render | output] side by side, the larger images
    reduced to the smallest size; a chunk of triptychs is composed by three launches and copied once."""
    from Evaluation.visual_eval import Reconstruct_Frames, tensor2im_batch
    from launches import observed
    mods = _fixed_modules(256)
    p = synth.tensor('frames/p', (3, 3, 256, 256), dist='uniform').to(dev())
    r = synth.tensor('frames/r', (3, 3, 256, 256), dist='uniform').to(dev())
    full, floats = Reconstruct_Frames(p, r, mods, chunk=2, return_float=True)
    assert len(full) == 3 and tuple(floats.shape) == (3, 3, 256, 256)
    short = Reconstruct_Frames(p, list(r[:2]), mods, chunk=2)
    assert len(short) == 2 and len(Reconstruct_Frames(list(p[:1]), r, mods, chunk=2)) == 1
    for a, b in zip(short, full):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(full[0], full[1]) and not np.array_equal(full[1], full[2])
    with observed() as rec:
        trip, tf = Reconstruct_Frames(p, r, mods, chunk=2, triptych=True, return_float=True)
    assert rec.count('tiles_to_canvas') == 3 * 2                          # two chunks, three source tensors each
    assert len(trip) == 3 and all(t.shape == (256, 768, 3) and t.dtype == np.uint8 for t in trip)
    side = [tensor2im_batch(t).cpu().numpy() for t in (p, r, tf)]
    for t in range(3):
        np.testing.assert_array_equal(trip[t], np.concatenate([s[t] for s in side], axis=1))
    assert torch.equal(tf, floats)
    # outputs smaller than the inputs: everything at the output's size
    G = _narrow_g()
    mods64 = (_FixedEncoder('tsr', (16, 4, 4), 0.5, 0.0).to(dev()), _FixedEncoder('w', (512,), 0.5, 0.0).to(dev()),
              _FixedEncoder('wp', (G.n_latent, 512), 0.2, 1.0).to(dev()), PinNoise(G))
    trip, tf = Reconstruct_Frames(p[:2], r[:2], mods64, triptych=True, return_float=True)
    assert all(t.shape == (64, 192, 3) for t in trip)
    side = [tensor2im_batch(_reduced(p[:2], 4)), tensor2im_batch(_reduced(r[:2], 4)), tensor2im_batch(tf)]
    for t in range(2):
        np.testing.assert_array_equal(trip[t], torch.cat([s[t] for s in side], 1).cpu().numpy())
    with pytest.raises(ValueError):
        Reconstruct_Frames(p, r, mods, chunk=0)


def test_gif_driver_equals_reconstruct_frames(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from Evaluation.visual_eval import Get_Multi_Photo_Multi_Render_Result, Load_GIF_As_Img_List, Reconstruct_Frames
    G = _narrow_g()
    mods = (_FixedEncoder('tsr', (16, 4, 4), 0.5, 0.0).to(dev()), _FixedEncoder('w', (512,), 0.5, 0.0).to(dev()),
            _FixedEncoder('wp', (G.n_latent, 512), 0.2, 1.0).to(dev()), PinNoise(G))

    def frames(n, base, step):
        out = [np.full((256, 256, 3), base + step * t, np.uint8) for t in range(n)]       # flat colours survive the palette
        for t, f in enumerate(out):
            f[32 * t:32 * t + 64, 16:200] = (250, 10 * t, base)
        return out

    def save(name, arrays):
        pil = [Image.fromarray(f) for f in arrays]
        pil[0].save(tmp_path / name, save_all=True, append_images=pil[1:], duration=40, loop=0)

    save('photo.gif', frames(4, 30, 50))
    save('render.gif', frames(3, 40, 60))

    def transform(img):
        a = torch.from_numpy(np.asarray(img.convert('RGB'), dtype=np.uint8).copy())
        return a.permute(2, 0, 1).float() / 127.5 - 1.0

    out = Get_Multi_Photo_Multi_Render_Result(str(tmp_path / 'photo.gif'), str(tmp_path / 'render.gif'), mods, transform,
                                              dev(), chunk=2)
    assert len(out) == 3 and all(o.dtype == np.uint8 and o.shape == (64, 64, 3) for o in out)      # the shorter GIF
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])
    p = torch.stack(Load_GIF_As_Img_List(str(tmp_path / 'photo.gif'), transform)).to(dev())
    r = Load_GIF_As_Img_List(str(tmp_path / 'render.gif'), transform)
    assert p.shape[0] == 4 and len(r) == 3
    ref = Reconstruct_Frames(p, r, mods, chunk=2)
    for a, b in zip(out, ref):
        np.testing.assert_array_equal(a, b)
