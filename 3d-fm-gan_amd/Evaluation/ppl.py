"""Perceptual path length in W space (reference Evaluation/ppl.py:37-137; the published StyleGAN2 script is the second
half of that file, :142-215).

    Generate_Interpolated_Image  :42-79    z -> w by the mapping network, e0 = lerp(w0, w1, t), e1 = lerp(w0, w1, t + eps),
                                           interleaved, then the Generator on [e] as latent styles
    Get_PPL_Score                :83-137   per batch: images -> (reduction to 256^2 when larger) -> LPIPS of each pair;
                                           mean of the distances between the 1st ('lower') and 99th ('higher') percentile

PPL_Distances gives the per-pair distances as one device tensor, PPL_Filter the filtered mean, Get_PPL_Score both with the
reference's signature.

What is different, on purpose:
  * nothing synchronises with the host inside the loop: the distances stay on the device and are transferred once, in
    PPL_Filter (the reference copies every batch's distances to the host);
  * the stage between the Generator and the VGG trunk (crop, reduction, split into the two halves, ScalingLayer, NHWC) is
    one HIP launch (op/ppl_input.py) wherever the kernel serves the batch and `percept` has forward_scaled and is in
    eval mode; otherwise the plain percept(image[::2], image[1::2]) after the reference's resize;
  * the mapping network is called directly (the reference wraps it in nn.DataParallel for every batch);
  * `percept` may be passed in (loaded weights); the reference builds lpips.PerceptualLoss inside, which downloads the
    pretrained blobs.  percept=None builds the module with its own initialisation: the blobs are not shipped, so such a
    score is a load figure, not a published one;
  * `crop`, `normalize` and `sampler` are the script half's --crop, its division by eps^2 and a hook for fixed samples;
    their defaults are the function half's behaviour.
Reference behaviour kept on purpose:
  * n_sample // batch_size batches of batch_size pairs each are evaluated: the reference computes a residual batch size
    and never uses it (its loop passes batch_size to every batch);
  * Get_PPL_Score does not divide by eps^2 (only the script half does: normalize=True);
  * n_sample < batch_size is a ValueError here (no batch at all: the reference fails inside numpy's percentile).
Out of scope: Z-space sampling with slerp (FID: Evaluation/fid.py; image projection: Evaluation/image_projection/).
"""
import numpy as np
import torch

from lpips import scaling_layer_of
from op.ppl_input import pair_input, pair_resize


def lerp(a, b, t):
    return a + (b - a) * t


def default_sampler(batch_index, batch_size, latent_dim, device):
    """(noise_z [2B, D], lerp_t [B]) drawn on the device in the reference's order: randn, then rand."""
    noise_z = torch.randn([batch_size * 2, latent_dim], device=device)
    lerp_t = torch.rand(batch_size, device=device)
    return noise_z, lerp_t


def Interpolated_Latents(style, noise_z, lerp_t, eps):
    """latent_e [2B, D]: rows 2p and 2p+1 are pair p's latents at t and t + eps (reference ppl.py:71-75)."""
    latent = style(noise_z)
    latent_t0, latent_t1 = latent[::2], latent[1::2]
    latent_e0 = lerp(latent_t0, latent_t1, lerp_t[:, None])
    latent_e1 = lerp(latent_t0, latent_t1, lerp_t[:, None] + eps)
    return torch.stack([latent_e0, latent_e1], 1).view(*latent.shape)


def PPL_Distances(generator, percept, n_sample, batch_size, eps, latent_dim, device, sampler=None, crop=False,
                  normalize=False, info_print=False, fuse=True):
    """Per-pair LPIPS distances [n_sample // batch_size * batch_size] as one device tensor, in batch order.
    generator: the Generator or a wrapper with `.module` (the mapping network is `.module.style` then); it is called as
    generator(noise_z=None, latent_styles=[latent_e], input_is_latent=True, noise=None).  percept: the distance,
    percept(pred, target) -> one value per sample.  sampler(batch_index, batch_size, latent_dim, device) ->
    (noise_z, lerp_t); default_sampler when None.  crop: the script's face crop before the reduction.  normalize: divide
    by eps^2.  fuse=False keeps the composite input stage (tests, tools/bench_ppl.py)."""
    if batch_size <= 0 or n_sample < batch_size:
        raise ValueError(f'PPL_Distances: n_sample {n_sample} gives no batch of {batch_size} pairs')
    sampler = sampler or default_sampler
    style = getattr(generator, 'module', generator).style
    scaling = scaling_layer_of(percept, 'forward_scaled')     # None: the fused input stage does not apply
    distances = []
    with torch.no_grad():
        for idx in range(n_sample // batch_size):
            if info_print:
                print('Evaluating Batch: ' + str(idx))
            noise_z, lerp_t = sampler(idx, batch_size, latent_dim, device)
            latent_e = Interpolated_Latents(style, noise_z, lerp_t, eps)
            image = generator(noise_z=None, latent_styles=[latent_e], input_is_latent=True, noise=None)
            if scaling is not None:
                in0, in1 = pair_input(image, scaling, crop=crop, fuse=fuse)
                dist = percept.forward_scaled(in0, in1)
            else:
                image = pair_resize(image, crop)
                dist = percept(image[::2], image[1::2])
            distances.append(dist.reshape(image.shape[0] // 2))
    distances = torch.cat(distances)
    return distances / (eps ** 2) if normalize else distances


def PPL_Filter(distances):
    """float64 mean of the distances within [1st percentile ('lower'), 99th percentile ('higher')]: one transfer to the
    host (reference ppl.py:126-134)."""
    d = distances.detach().to('cpu').numpy() if torch.is_tensor(distances) else np.asarray(distances)
    lo = np.percentile(d, 1, method='lower')
    hi = np.percentile(d, 99, method='higher')
    kept = np.extract(np.logical_and(lo <= d, d <= hi), d)
    return np.mean(kept, dtype=np.float64)


def Get_PPL_Score(generator, n_sample, batch_size, eps, latent_dim, device, gpu_device_ids=None, info_print=False,
                  percept=None, **kw):
    """The PPL score of a model, with the reference's signature (gpu_device_ids is accepted and unused: one device).
    percept: the perceptual distance with loaded weights; None builds lpips.PerceptualLoss(model='net-lin', net='vgg') in
    channels_last on `device` with its own initialisation.  **kw: sampler, crop, normalize, fuse of PPL_Distances."""
    if percept is None:
        import lpips
        percept = lpips.PerceptualLoss(model='net-lin', net='vgg').to(device).to(memory_format=torch.channels_last)
    return PPL_Filter(PPL_Distances(generator, percept, n_sample, batch_size, eps, latent_dim, device,
                                    info_print=info_print, **kw))
