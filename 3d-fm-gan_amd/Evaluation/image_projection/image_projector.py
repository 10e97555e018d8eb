"""Image projection: embed a photograph into W or W+ of a Generator by optimising the latent and the per-layer noise maps
against mse + LPIPS (reference Evaluation/image_projection/image_projector.py), and the PSNR / LPIPS helpers that score
such projections.

    Get_Avg_W_as_Latent   :30-59     mean of the mapping network over 1000 samples, as [1, 512] or [1, n_latent, 512]
    Image_Projector       :67-147    (input_img, output_img): the image of the average latent and the projected image
    Downsample_Image_256, Get_LPIPS_Model_Image, psnr, Get_PSNR_Model_Image   :155-219

What is different, on purpose:
  * target_im may also be a float tensor [B, 3, S, S] in [-1, 1] (the reference takes PIL images only);
  * torchvision's ToTensor + Normalize(0.5, 0.5) is Util.image_io.images_to_tensor on the GPU and the same arithmetic in
    torch on the CPU;
  * a Generator behind `.module` is recognised by that attribute (the reference looks for 'module' in the first
    state_dict key) and its mapping network is called directly (the reference wraps it in nn.DataParallel);
  * the Generator's requires_grad flags and training mode are restored on return (the reference leaves it frozen and
    in eval mode); its parameters are never written;
  * the reference's first optimiser, its third-party FullBatchLBFGS(lr=1), is LBFGS.py here and is asked for as
    opt='FullBatchLBFGS'.  The reference's spelling opt='LBFGS' still raises NotImplementedError (its message names the
    new spelling).  opt='Adam' is the reference's; any torch.optim.Optimizer class or factory may be passed instead of
    a name, lambda p: LBFGS.FullBatchLBFGS(p, lr=1) among them;
  * `criterion` None builds project.ImageReconstructionLoss(loss='mse+lpips') without pretrained LPIPS weights (a load
    figure: see project.py); pass a criterion built with percept= for real scores.
"""
import math

import numpy as np
import torch

from . import LBFGS, project

NUM_AVG_SAMPLES = 1000


def _plain(generator):
    return getattr(generator, 'module', generator)


def img_transform(images, device):
    """transforms.ToTensor() + Normalize([0.5] * 3, [0.5] * 3) of a list of equally sized RGB images (PIL images or
    uint8 HWC arrays) -> float32 [B, 3, H, W] on `device`."""
    u8 = torch.from_numpy(np.stack([np.asarray(im, dtype=np.uint8) for im in images])).to(device)
    if u8.ndim != 4 or u8.shape[3] != 3:
        raise ValueError(f'img_transform: expected RGB images of one size, got a batch of shape {tuple(u8.shape)}')
    if u8.is_cuda:
        from Util import image_io
        return image_io.images_to_tensor(u8.contiguous(), 0.5, 0.5)
    return (u8.permute(0, 3, 1, 2).to(torch.float32) / 255 - 0.5) / 0.5


def Get_Avg_W_as_Latent(generator, device, per_layer_W, is_generator_DPmodule=False):
    """The average latent of a generator from 1000 samples of its mapping network: [1, n_latent, 512] when per_layer_W,
    else [1, 512].  is_generator_DPmodule is accepted for the reference's signature; `.module` is found either way."""
    g = _plain(generator)
    with torch.no_grad():
        noise_z = torch.randn(NUM_AVG_SAMPLES, g.style_dim).to(device)
        avg_W = torch.mean(g.style(noise_z), axis=0)
        if per_layer_W is True:
            return avg_W.repeat((g.num_layers + 1, 1)).unsqueeze(0)
        return avg_W.reshape(1, -1)


def Image_Projector(generator, device, per_layer_W, target_im, opt, num_iters=500, print_iters=20, criterion=None):
    """Project target_im (a PIL image, a list of them, or a float tensor [B, 3, S, S]) with `generator`; returns
    (input_img, output_img) on the CPU: the image of the starting point (the average latent with fresh noise maps) and
    the image after num_iters + 1 optimisation steps."""
    if opt == 'LBFGS':
        raise NotImplementedError("Image_Projector: opt='LBFGS' is the reference's third-party FullBatchLBFGS, which is "
                                  "asked for as opt='FullBatchLBFGS' here; or use opt='Adam' or pass a "
                                  "torch.optim.Optimizer class")
    if opt == 'FullBatchLBFGS':
        make_optimizer = lambda params: LBFGS.FullBatchLBFGS(params, lr=1)     # noqa: E731
    elif opt == 'Adam':
        make_optimizer = lambda params: torch.optim.Adam(params, lr=0.01)      # noqa: E731
    elif callable(opt):
        make_optimizer = opt
    else:
        raise ValueError(f"Image_Projector: opt {opt!r}: expected 'FullBatchLBFGS', 'Adam' or a callable params -> "
                         f"torch.optim.Optimizer")
    g = _plain(generator)
    params = list(generator.parameters())
    was = [p.requires_grad for p in params], generator.training
    for p in params:
        p.requires_grad = False
    generator.eval()
    try:
        if torch.is_tensor(target_im):
            target = target_im.detach().to(device=device, dtype=torch.float32).contiguous()
            if target.ndim != 4 or target.shape[1] != 3:
                raise ValueError(f'Image_Projector: target tensor {tuple(target.shape)}: expected [B, 3, S, S]')
        else:
            target = img_transform(target_im if isinstance(target_im, list) else [target_im], device)
        avg_W = Get_Avg_W_as_Latent(generator, device, per_layer_W)
        avg_W = torch.repeat_interleave(avg_W, target.shape[0], dim=0)
        avg_W.requires_grad = True
        noises = g.make_noise()
        for noise in noises:
            noise.requires_grad = True
        input_kwargs = {'noise_z': None, 'input_is_latent': True, 'latent_styles': [avg_W], 'noise': noises}
        with torch.no_grad():
            input_img = generator(**input_kwargs).detach().cpu()
        if criterion is None:
            criterion = project.ImageReconstructionLoss(device=device, loss='mse+lpips')
        optimizer = make_optimizer([avg_W] + noises)
        project.optimize(model=generator, input_kwargs=input_kwargs, targets={'target': target, 'mask': None},
                         criterion=criterion, optimizer=optimizer, iterations=num_iters, print_iterations=print_iters,
                         device=device)
        with torch.no_grad():
            output_img = generator(**input_kwargs).detach().cpu()
    finally:
        for p, flag in zip(params, was[0]):
            p.requires_grad = flag
        generator.train(was[1])
    return input_img, output_img


# ---------------------------------------- Image Projection Evaluation ----------------------------------------
def Downsample_Image_256(im_tensor):
    """Halve the image (bilinear, align_corners=False) until it is no larger than 256."""
    while im_tensor.shape[2] > 256:
        im_tensor = torch.nn.functional.interpolate(im_tensor, scale_factor=1 / 2, mode='bilinear', align_corners=False)
    return im_tensor


def Get_LPIPS_Model_Image(output_img_tensor_list, target_img_tensor_list, lpips_percept):
    """LPIPS of every (output, target) pair: output_img_tensor_list holds num_model * num_img [1, C, H, W] tensors, model
    by model; returns one list of num_img floats per model.  As in the reference the target is the first argument."""
    num_img = len(target_img_tensor_list)
    assert len(output_img_tensor_list) % num_img == 0
    scores = []
    with torch.no_grad():
        for i in range(len(output_img_tensor_list) // num_img):
            scores.append([float(lpips_percept(Downsample_Image_256(target_img_tensor_list[j]),
                                               Downsample_Image_256(output_img_tensor_list[j + num_img * i])))
                           for j in range(num_img)])
    return scores


def psnr(img1, img2):
    mse = np.mean((img1 - img2) ** 2)
    if mse == 0:
        return 100
    return 20 * math.log10(255.0 / math.sqrt(mse))


def Get_PSNR_Model_Image(output_img_list, target_img_list):
    """PSNR of every (output, target) pair of numpy images on the 0..255 scale; the lists as in Get_LPIPS_Model_Image."""
    num_img = len(target_img_list)
    assert len(output_img_list) % num_img == 0
    return [[float(psnr(target_img_list[j], output_img_list[j + num_img * i])) for j in range(num_img)]
            for i in range(len(output_img_list) // num_img)]
