"""Output side of the path (reference: Evaluation/visual_eval.py): `tensor2im` (:24-38) and the re-animation driver
(:147-205: one photo, the frames of a render GIF) on the photo-encoded-once path of Util/network_util.py.  The other
drivers of the reference file (grids, video writers) are evaluation tooling and not provided."""
import numpy as np
import torch

from op import _native
from Util.network_util import Encode_Photo, Forward_Inference_Reanimate


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
        raise ValueError('model_modules = (E_Tsr, E_W, E_W_Plus, g_ema): the 3-encoder scheme is the one this build provides')
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
