"""Output side of the path (reference: Evaluation/visual_eval.py): `tensor2im` (:24-38), the sample pickers (:40-83),
the sample grid (:86-142, and as one picture composed on the device: Batch_Eval_Sheet), the re-animation driver
(:147-205: one photo, the frames of a render GIF) on the photo-encoded-once path of Util/network_util.py, the video
reconstruction driver (:265-302: a photo GIF and a render GIF, frame by frame, in chunks) and the two test drivers that
write result GIFs (:207-263, :304-340).  Every image leaves the device as uint8: one copy per source tensor, one per
sheet, one per chunk of triptychs (op/canvas.py).  These drivers take the four modules of the 3-encoder scheme; the
2-encoder scheme (three modules) has the re-animation pair Reanimate_Frames_2_Encoder /
Get_Single_Photo_Multi_Render_Result_2_Encoder of its own."""
import os
import random

import numpy as np
import torch

from op import _native
from op.canvas import sheet_layout, tiles_to_canvas
from Util.network_util import (Encode_Photo, Encode_Photo_2_Encoder, Forward_Inference_3_Encoder,
                               Forward_Inference_Reanimate, Forward_Inference_Reanimate_2_Encoder)

VAL_SET_LEN = 3
NUM_IMG_PER_ID = 7
_FOUR_MODULES = 'model_modules = (E_Tsr, E_W, E_W_Plus, g_ema): the 3-encoder scheme is the one this build provides'


def tensor2im(image_tensor, imtype=np.uint8, cent=1., factor=255. / 2.):
    """[-1,1] image tensor -> numpy uint8 HWC image of the FIRST sample, as the reference does; the clip/scale/cast
    and the CHW->HWC transposition run in one GPU pass (`tensor2im_batch` converts every sample)."""
    img = _native.tensor_to_images(image_tensor[:1].float(), cent, factor)[0].cpu().numpy()
    return img.astype(imtype)


def tensor2im_batch(image_tensor, cent=1., factor=255. / 2.):
    """uint8 [B,H,W,3] GPU tensor for the whole batch."""
    return _native.tensor_to_images(image_tensor.float(), cent, factor)


def Reanimate_Frames(p_input, r_frames, model_modules, chunk=8, return_float=False, **kwargs):
    """One photo [1,3,256,256] re-animated by render frames ([N,3,256,256], or a list of [3,H,W] / [1,3,H,W] tensors):
    list of N uint8 HWC arrays, in frame order.  The photo is encoded once; the frames run `chunk` at a time (the last
    chunk is shorter).  model_modules = (E_Tsr, E_W, E_W_Plus, g_ema), the reference's order; kwargs: tsr_encode,
    sliced_layer, use_tanh, noise, randomize_noise.  return_float: also the float frames [N,3,S,S] (on the GPU)."""
    if len(model_modules) != 4:
        raise ValueError(_FOUR_MODULES)
    if chunk < 1:
        raise ValueError('chunk must be positive')
    E_Tsr, E_W, E_W_Plus, g_ema = model_modules
    if not torch.is_tensor(r_frames):
        r_frames = torch.stack([f.reshape(f.shape[-3:]) for f in r_frames], 0)
    r_frames = r_frames.to(p_input.device)
    tsr_encode = kwargs.pop('tsr_encode', 'Photo Image')
    code = Encode_Photo(p_input, E_Tsr, E_W_Plus, tsr_encode)
    images, floats = [], []
    for i in range(0, r_frames.shape[0], chunk):
        out = Forward_Inference_Reanimate(code, r_frames[i:i + chunk].contiguous(), E_Tsr, E_W, g_ema,
                                          tsr_encode=tsr_encode, **kwargs)
        images += list(tensor2im_batch(out).cpu().numpy())
        if return_float:
            floats.append(out.clone())      # a graphed or workspace-backed output may be overwritten by the next chunk
    return (images, torch.cat(floats, 0)) if return_float else images


def Load_GIF_As_Img_List(gif_path, transform):
    """Every frame of a GIF, converted to RGB and passed through `transform` (Evaluation/visual_eval.py:188-205)."""
    from PIL import Image
    with Image.open(gif_path) as gif:
        frames = []
        for i in range(gif.n_frames):
            gif.seek(i)
            frames.append(transform(gif.convert('RGB')))
    return frames


def Get_Single_Photo_Multi_Render_Result(photo_img_png_path, render_img_gif_path, model_modules, transform, device,
                                         **kwargs):
    """One photo (.png) re-animated by the frames of a render .gif (Evaluation/visual_eval.py:147-186): list of uint8
    HWC images, one per frame.  kwargs as Reanimate_Frames (chunk included)."""
    from PIL import Image
    with Image.open(photo_img_png_path) as img:
        p_input = transform(img).to(device).unsqueeze(0)
    return Reanimate_Frames(p_input, Load_GIF_As_Img_List(render_img_gif_path, transform), model_modules, **kwargs)


def Reanimate_Frames_2_Encoder(p_input, r_frames, model_modules, chunk=8, return_float=False, **kwargs):
    """Reanimate_Frames for the 2-encoder scheme: model_modules = (E_Tsr, E_W, g_ema) (tensor encoder, modulation
    encoder, generator); kwargs: mod_encode, co_modulation, sliced_layer, use_tanh, noise, randomize_noise.  The photo
    is encoded once (Encode_Photo_2_Encoder), the frames run `chunk` at a time, one uint8 copy per chunk."""
    if len(model_modules) != 3:
        raise ValueError('model_modules = (E_Tsr, E_W, g_ema): the three modules of the 2-encoder scheme')
    if chunk < 1:
        raise ValueError('chunk must be positive')
    E_Tsr, E_W, g_ema = model_modules
    if not torch.is_tensor(r_frames):
        r_frames = torch.stack([f.reshape(f.shape[-3:]) for f in r_frames], 0)
    r_frames = r_frames.to(p_input.device)
    mod_encode = kwargs.pop('mod_encode', 'Render Image')
    co_modulation = kwargs.pop('co_modulation', None)
    code = Encode_Photo_2_Encoder(p_input, E_Tsr, E_W, mod_encode, co_modulation)
    images, floats = [], []
    for i in range(0, r_frames.shape[0], chunk):
        out = Forward_Inference_Reanimate_2_Encoder(code, r_frames[i:i + chunk].contiguous(), E_Tsr, E_W, g_ema,
                                                    mod_encode=mod_encode, co_modulation=co_modulation, **kwargs)
        images += list(tensor2im_batch(out).cpu().numpy())
        if return_float:
            floats.append(out.clone())      # a workspace-backed output may be overwritten by the next chunk
    return (images, torch.cat(floats, 0)) if return_float else images


def Get_Single_Photo_Multi_Render_Result_2_Encoder(photo_img_png_path, render_img_gif_path, model_modules, transform,
                                                   device, **kwargs):
    """Get_Single_Photo_Multi_Render_Result for the 2-encoder scheme; kwargs as Reanimate_Frames_2_Encoder."""
    from PIL import Image
    with Image.open(photo_img_png_path) as img:
        p_input = transform(img).to(device).unsqueeze(0)
    return Reanimate_Frames_2_Encoder(p_input, Load_GIF_As_Img_List(render_img_gif_path, transform), model_modules,
                                      **kwargs)


# ----------------------------------------------------------------------------------------------- sample pickers
def Get_Real_Img_Val_Sample(real_img_val_list, transform, num_faces, device):
    """Real photos with their rendered faces for the visual validation (Evaluation/visual_eval.py:40-56): `num_faces`
    files of the list, each an .npy stack [photo, render, partner renders...]; a set is the photo, its render and one
    partner render.  The same draws from np.random / random in the same order as the reference: a seeded run picks
    the same files and partners.  Returns the flat list of [1,3,H,W] tensors on `device`, VAL_SET_LEN per face."""
    from PIL import Image
    sel_real_img_file = np.random.choice(real_img_val_list, size=num_faces, replace=False)
    real_img_val_sets = []
    for img_file in sel_real_img_file:
        img_np = list(np.load(img_file))
        test_set = img_np[:2] + [random.choice(img_np[2:])]
        real_img_val_sets += [transform(Image.fromarray(img)).unsqueeze(dim=0).to(device) for img in test_set]
    return real_img_val_sets


def Syn_Img_Val_Indices(dataset_len, num_faces):
    """The dataset indices Get_Syn_Img_Val_Sample loads (:68-72): num_faces identities, num_faces of the
    NUM_IMG_PER_ID images of each, drawn from np.random in the reference's order."""
    num_id = dataset_len // NUM_IMG_PER_ID
    load_idx = []
    for person_id in np.random.choice(num_id, num_faces):
        idx = person_id * NUM_IMG_PER_ID + np.random.choice(NUM_IMG_PER_ID, num_faces)
        load_idx += list(idx)
    return load_idx


def Get_Syn_Img_Val_Sample(synface_dataset, num_faces, device):
    """Synthetic images with their renders for the visual validation (Evaluation/visual_eval.py:59-83): of the loaded
    (image, render) pairs every even one contributes both, every odd one its render — sets of VAL_SET_LEN at
    num_faces = 2, the reference's setting."""
    syn_img_val_sets = []
    for i, idx in enumerate(Syn_Img_Val_Indices(len(synface_dataset), num_faces)):
        g_img, r_img = synface_dataset[idx]
        if i % 2 == 0:
            syn_img_val_sets += [g_img.unsqueeze(dim=0).to(device), r_img.unsqueeze(dim=0).to(device)]
        else:
            syn_img_val_sets += [r_img.unsqueeze(dim=0).to(device)]
    return syn_img_val_sets


# ----------------------------------------------------------------------------------------------- sample grid
def _eval_set_forward(g_input, r_input_list, generative_model, kwargs):
    """(photo [1,3,h,w], renders [R,3,h,w], outputs [R,3,S,S]) of one set, float, on the GPU: the photo encoded once,
    all renders in one forward.  As tensor2im, the first sample of every input is the one that counts."""
    if len(generative_model) != 4:
        raise ValueError(_FOUR_MODULES)
    E_Tsr, E_W, E_W_Plus, g_ema = generative_model
    kwargs = dict(kwargs)
    tsr_encode = kwargs.pop('tsr_encode', 'Photo Image')
    photo = g_input[:1].float()
    renders = torch.cat([r[:1].float() for r in r_input_list], 0).contiguous()
    code = Encode_Photo(photo, E_Tsr, E_W_Plus, tsr_encode)
    out = Forward_Inference_Reanimate(code, renders, E_Tsr, E_W, g_ema, tsr_encode=tsr_encode, **kwargs)
    return photo, renders, out


def Get_Single_Eval_Result(g_input, r_input_list, generative_model, **kwargs):
    """The reference's list [photo, render_1, out_1, render_2, out_2, ...] of uint8 HWC arrays for one photo and its
    renders (Evaluation/visual_eval.py:86-118).  kwargs: tsr_encode, sliced_layer, use_tanh, noise, randomize_noise."""
    photo, renders, out = _eval_set_forward(g_input, r_input_list, generative_model, kwargs)
    photo, renders, out = (tensor2im_batch(t).cpu().numpy() for t in (photo, renders, out))
    img_plot_list = [photo[0]]
    for k in range(renders.shape[0]):
        img_plot_list += [renders[k], out[k]]
    return img_plot_list


def Get_Batch_Eval_Result(eval_img_set, generative_model, **kwargs):
    """Get_Single_Eval_Result over the sets of VAL_SET_LEN images, as one flat list (:120-142)."""
    num_test_set = len(eval_img_set) // VAL_SET_LEN
    img_result_plot_list = []
    for i in range(num_test_set):
        test_set = eval_img_set[i * VAL_SET_LEN: (i + 1) * VAL_SET_LEN]
        img_result_plot_list += Get_Single_Eval_Result(test_set[0], test_set[1:], generative_model, **kwargs)
    return img_result_plot_list


def _slot_ratio(t, tile, what):
    if t.shape[-1] != t.shape[-2] or t.shape[-1] not in (tile, 2 * tile, 4 * tile):
        raise ValueError(f'{what} of {tuple(t.shape[-2:])} into tiles of side {tile}: the ratio must be 1, 2 or 4')


def Batch_Eval_Sheet(eval_img_set, generative_model, tile=256, gap=8, margin=8, background=255, **kwargs):
    """The pictures of Get_Batch_Eval_Result as one uint8 [H, W, 3] tensor on the GPU: one row per set, 1 + 2 *
    (VAL_SET_LEN - 1) columns (photo, render_1, out_1, render_2, out_2) — the reference's figure
    (train_3_encoder.py:688-706) without matplotlib.  Tiles of side `tile`; an image 2 or 4 times as large is reduced
    by the kernel (bilinear, align_corners=False), any other ratio raises ValueError.  One launch per source tensor
    (photos, renders, outputs), nothing copied to the host."""
    num_test_set = len(eval_img_set) // VAL_SET_LEN
    if num_test_set < 1:
        raise ValueError(f'Batch_Eval_Sheet: {len(eval_img_set)} images are no set of {VAL_SET_LEN}')
    n_col = 1 + 2 * (VAL_SET_LEN - 1)
    canvas_h, canvas_w, yx = sheet_layout(num_test_set, n_col, tile, gap, margin)
    yx = yx.reshape(num_test_set, n_col, 2)
    photos, renders, outs = [], [], []
    for i in range(num_test_set):
        test_set = eval_img_set[i * VAL_SET_LEN: (i + 1) * VAL_SET_LEN]
        photo, render, out = _eval_set_forward(test_set[0], test_set[1:], generative_model, kwargs)
        for t, what in ((photo, 'photo'), (render, 'renders'), (out, 'outputs')):
            _slot_ratio(t, tile, f'Batch_Eval_Sheet: {what}')
        photos.append(photo)
        renders.append(render)
        outs.append(out.clone())    # a graphed or workspace-backed output may be overwritten by the next set
    canvas = torch.full((canvas_h, canvas_w, 3), int(background), dtype=torch.uint8, device=photos[0].device)
    tiles_to_canvas(torch.cat(photos, 0), canvas, yx[:, 0], tile)
    tiles_to_canvas(torch.cat(renders, 0), canvas, yx[:, 1::2].reshape(-1, 2), tile)
    tiles_to_canvas(torch.cat(outs, 0), canvas, yx[:, 2::2].reshape(-1, 2), tile)
    return canvas


# ----------------------------------------------------------------------------------------------- video reconstruction
def _frame_batch(frames, device):
    if not torch.is_tensor(frames):
        frames = torch.stack([f.reshape(f.shape[-3:]) for f in frames], 0)
    return frames.to(device).float()


def Reconstruct_Frames(p_frames, r_frames, model_modules, chunk=8, triptych=False, return_float=False, tile=None,
                       **kwargs):
    """A video reconstructed frame by frame: frame t is Forward_Inference_3_Encoder(p_t, r_t, ...), `chunk` frames per
    call over min(len(p_frames), len(r_frames)) frames (the reference's zip, Evaluation/visual_eval.py:290-300).
    p_frames / r_frames: [N,3,H,W] tensors (p_frames on the GPU) or lists of [3,H,W] / [1,3,H,W] tensors.  Returns the
    list of uint8 HWC arrays, in frame order.  triptych: each frame is [photo | render | output], composed on the
    device into a [chunk, tile, 3 * tile, 3] canvas batch and copied once per chunk; `tile` defaults to the smallest of
    the three sizes, larger images are reduced by 2 or 4 (any other ratio: ValueError).  model_modules = (E_Tsr, E_W,
    E_W_Plus, g_ema); kwargs: tsr_encode, sliced_layer, use_tanh.  return_float: also the float frames [N,3,S,S]."""
    if len(model_modules) != 4:
        raise ValueError(_FOUR_MODULES)
    if chunk < 1:
        raise ValueError('chunk must be positive')
    E_Tsr, E_W, E_W_Plus, g_ema = model_modules
    device = p_frames.device if torch.is_tensor(p_frames) else p_frames[0].device     # the photo frames name the device
    p_frames, r_frames = _frame_batch(p_frames, device), _frame_batch(r_frames, device)
    n = min(p_frames.shape[0], r_frames.shape[0])
    images, floats = [], []
    for i in range(0, n, chunk):
        p, r = p_frames[i:min(i + chunk, n)].contiguous(), r_frames[i:min(i + chunk, n)].contiguous()
        with torch.no_grad():
            out = Forward_Inference_3_Encoder(p, r, E_Tsr, E_W, E_W_Plus, g_ema, **kwargs)
        if triptych:
            side = int(tile) if tile is not None else min(p.shape[-1], r.shape[-1], out.shape[-1])
            c = p.shape[0]
            canvas = torch.empty((c, side, 3 * side, 3), dtype=torch.uint8, device=out.device)
            for col, (t, what) in enumerate(((p, 'photo frames'), (r, 'render frames'), (out, 'outputs'))):
                _slot_ratio(t, side, f'Reconstruct_Frames: {what}')
                tiles_to_canvas(t.contiguous(), canvas, [(k, 0, col * side) for k in range(c)], side)
            images += list(canvas.cpu().numpy())
        else:
            images += list(tensor2im_batch(out).cpu().numpy())
        if return_float:
            floats.append(out.clone())      # a graphed or workspace-backed output may be overwritten by the next chunk
    if return_float:
        return images, (torch.cat(floats, 0) if floats else torch.empty((0, 3, 0, 0), device=device))
    return images


def Get_Multi_Photo_Multi_Render_Result(photo_img_gif_path, render_img_gif_path, model_modules, transform, device,
                                        **kwargs):
    """The frames of a photo .gif reconstructed under the frames of a render .gif (Evaluation/visual_eval.py:265-302),
    up to the shorter of the two: list of uint8 HWC images.  kwargs as Reconstruct_Frames (chunk, triptych included)."""
    if len(model_modules) != 4:
        raise ValueError(_FOUR_MODULES)
    p_input_list = [t.to(device) for t in Load_GIF_As_Img_List(photo_img_gif_path, transform)]
    r_input_list = Load_GIF_As_Img_List(render_img_gif_path, transform)
    return Reconstruct_Frames(torch.stack(p_input_list, 0), r_input_list, model_modules, **kwargs)


# ----------------------------------------------------------------------------------------------- test drivers
def Get_Img_Path_Single_Factor_Test(test_dir):
    """(photo .png, render .gif) file-name pairs of a directory: a gif belongs to the photo whose stem it contains
    (Evaluation/visual_eval.py:207-225)."""
    photo_img_files = [file for file in os.listdir(test_dir) if '.png' in file]
    gif_img_files = [file for file in os.listdir(test_dir) if '.gif' in file]
    test_list = []
    for gif_file in gif_img_files:
        for photo_file in photo_img_files:
            if photo_file[:-4] in gif_file:
                test_list.append((photo_file, gif_file))
    return test_list


def Get_Img_Path_Video_Test(test_dir):
    """The two pairs of a video directory: (its .png, render_img.gif) and (photo_img.gif, render_img.gif) (:251-263)."""
    photo_img_file = [file for file in os.listdir(test_dir) if '.png' in file][0]
    return [(photo_img_file, 'render_img.gif'), ('photo_img.gif', 'render_img.gif')]


def Save_GIF(result_file_path, img_list):
    """imageio.mimsave where imageio is installed (what the reference calls), Pillow otherwise."""
    try:
        import imageio
    except ImportError:
        from PIL import Image
        pil = [Image.fromarray(np.asarray(img)) for img in img_list]
        pil[0].save(result_file_path, save_all=True, append_images=pil[1:], loop=0)
        return
    imageio.mimsave(result_file_path, img_list)


def Test_Single_Factor_Editing(test_dir, save_dir, model_name, model_modules, transform, device, **kwargs):
    """Every (photo, render gif) pair of test_dir re-animated and written to save_dir as
    '<model_name>_result_<gif name>' (Evaluation/visual_eval.py:227-249).  Returns the written paths."""
    written = []
    for test_pair in Get_Img_Path_Single_Factor_Test(test_dir):
        output_img_list = Get_Single_Photo_Multi_Render_Result(os.path.join(test_dir, test_pair[0]),
                                                               os.path.join(test_dir, test_pair[1]), model_modules,
                                                               transform, device, **kwargs)
        result_file_path = os.path.join(save_dir, model_name + '_result_' + test_pair[1])
        Save_GIF(result_file_path, output_img_list)
        written.append(result_file_path)
    return written


def Test_Video_Reconstruction_Reanimation(test_dir, save_dir, video_name, model_name, model_modules, transform, device,
                                          **kwargs):
    """The re-animation and the reconstruction of one video directory, written to save_dir under the reference's names
    (Evaluation/visual_eval.py:304-340).  Returns the two written paths."""
    test_pair_list = Get_Img_Path_Video_Test(test_dir)
    output_img_list = Get_Single_Photo_Multi_Render_Result(os.path.join(test_dir, test_pair_list[0][0]),
                                                           os.path.join(test_dir, test_pair_list[0][1]), model_modules,
                                                           transform, device, **kwargs)
    reanimation = os.path.join(save_dir, model_name + '_' + video_name + '_reanimation_' +
                               test_pair_list[0][0].replace('.png', '.gif'))
    Save_GIF(reanimation, output_img_list)
    output_img_list = Get_Multi_Photo_Multi_Render_Result(os.path.join(test_dir, test_pair_list[1][0]),
                                                          os.path.join(test_dir, test_pair_list[1][1]), model_modules,
                                                          transform, device, **kwargs)
    reconstruction = os.path.join(save_dir, model_name + '_' + video_name + '_reconstruction_' + test_pair_list[1][0])
    Save_GIF(reconstruction, output_img_list)
    return [reanimation, reconstruction]
