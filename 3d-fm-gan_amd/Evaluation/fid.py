"""Frechet Inception distance of a generator (reference Evaluation/fid.py:28-130).

    extract_feature_from_samples  :28-47    the reference's loop and signature; returns CPU features (kept for parity)
    calc_fid                      :50-73    |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2)
    Get_Model_FID_Score           :76-130   the one-button wrapper

What is different, on purpose:
  * Sample_Statistics runs the same loop without touching the host: every batch's features go into running float64
    moments on the device (op/fid_stats.py, one HIP launch per batch on the fp64 matrix instruction); the reference copies
    every batch to the host and runs np.cov over [n_sample, 2048] at the end;
  * the stage between the Generator and the network (resampling to 299^2, normalisation, channels_last) is one HIP launch
    (op/inception_input.py) wherever the kernel serves the batch; the network runs with BatchNorm folded
    (Evaluation/inception.py);
  * calc_fid takes tr sqrt(S1 S2) as the sum of the square roots of the eigenvalues of S1^(1/2) S2 S1^(1/2) (the same
    spectrum as S1 S2, but symmetric positive semi-definite: two torch.linalg.eigh in float64 on the host, negative
    round-off clamped to 0).  The reference's scipy.linalg.sqrtm of the unsymmetric product needs scipy, may return a
    complex matrix, and falls back to an eps offset when singular; here nothing can become complex or non-finite, so
    `eps` is accepted and unused;
  * neither the Inception weights nor the FFHQ statistics pickles are shipped: `inception` (or
    load_patched_inception_v3(weights)) and `real_stats` are the caller's.  inception=None builds the network with its
    own initialisation, whose score is a load figure, not an FID;
  * one process per GPU: no nn.DataParallel (gpu_device_ids is accepted and unused); per-GPU states combine with
    Feature_Statistics.merge.
FID_FUSE = False (or FMGAN_NO_FID_FUSE=1) selects the composite for both kernels: the baseline of profiles/fid.md.
"""
import os
import pickle

import numpy as np
import torch

from op.fid_stats import Feature_Statistics

from .calc_inception import features_of, load_patched_inception_v3

FID_FUSE = os.environ.get('FMGAN_NO_FID_FUSE', '0') != '1'

# the files the reference's Get_Model_FID_Score opens, relative to its Evaluation/ directory
REFERENCE_STATS_FILES = {256: 'inception_ffhq_embed/self_ffhq_256_inception_embeddings_eval_mode.pkl',
                         1024: 'inception_ffhq_embed/self_ffhq_1024_inception_embeddings_eval_mode.pkl'}


def batch_split(n_sample, batch_size):
    """The reference's split: n_batch - 1 batches of batch_size and a last one of what remains (fid.py:32-34)."""
    n_batch = n_sample // batch_size
    if batch_size <= 0 or n_batch < 1:
        raise ValueError(f'n_sample {n_sample} gives no batch of {batch_size}')
    return [batch_size] * (n_batch - 1) + [n_sample - (n_batch - 1) * batch_size]


def default_sampler(batch_index, batch, latent_dim, device):
    return torch.randn(batch, latent_dim, device=device)


def _batches(generator, inception, truncation, truncation_latent, batch_size, n_sample, device, sampler, fuse,
             info_print):
    """Yields every batch's [batch, D] features, in the reference's order."""
    sampler = sampler or default_sampler
    with torch.no_grad():
        generator.eval()
        inception.eval()
        for idx, batch in enumerate(batch_split(n_sample, batch_size)):
            if info_print:
                print('Processing Batch: ' + str(idx))
            latent = sampler(idx, batch, 512, device)
            img = generator([latent], truncation=truncation, truncation_latent=truncation_latent)
            yield features_of(inception, img, fuse)


def extract_feature_from_samples(generator, inception, truncation, truncation_latent, batch_size, n_sample, device,
                                 info_print=False, sampler=None):
    """[n_sample, D] features on the CPU (one transfer per batch, as the reference)."""
    feats = [f.to('cpu') for f in _batches(generator, inception, truncation, truncation_latent, batch_size, n_sample,
                                           device, sampler, FID_FUSE, info_print)]
    return torch.cat(feats, 0)


def Sample_Statistics(generator, inception, truncation, truncation_latent, batch_size, n_sample, device, sampler=None,
                      fuse=True, info_print=False):
    """The Feature_Statistics of n_sample generated images, by the reference's loop; nothing synchronises inside it.
    sampler(batch_index, batch, 512, device) -> latent z [batch, 512]; torch.randn when None."""
    stats = None
    for feat in _batches(generator, inception, truncation, truncation_latent, batch_size, n_sample, device, sampler, fuse,
                         info_print):
        if stats is None:
            stats = Feature_Statistics(feat.shape[1], feat.device, fuse=fuse)
        stats.update(feat)
    return stats


def _f64(a):
    if torch.is_tensor(a):
        return a.detach().to('cpu', torch.float64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _psd_eigh(m):
    """Eigenvalues (negative round-off clamped to 0) and eigenvectors of the symmetric part of m."""
    lam, vec = torch.linalg.eigh((m + m.T) / 2)
    return lam.clamp_min(0), vec


def calc_fid(sample_mean, sample_cov, real_mean, real_cov, eps=1e-6):
    """The FID of two Gaussians given as mean [D] and covariance [D, D] (numpy arrays or tensors), as a float."""
    mu1, mu2, s1, s2 = _f64(sample_mean), _f64(real_mean), _f64(sample_cov), _f64(real_cov)
    lam1, v1 = _psd_eigh(s1)
    root1 = (v1 * lam1.sqrt()) @ v1.T
    lam, _ = _psd_eigh(root1 @ s2 @ root1)
    mean_diff = mu1 - mu2
    trace = torch.trace(s1) + torch.trace(s2) - 2 * lam.sqrt().sum()
    return float(mean_diff @ mean_diff + trace)


def load_real_stats(real_stats, img_size=None):
    """(mean, cov) from a dict or the path of a pickle with the fields `mean` and `cov`."""
    if real_stats is None:
        want = REFERENCE_STATS_FILES.get(img_size, ' or '.join(REFERENCE_STATS_FILES.values()))
        raise ValueError(f'Get_Model_FID_Score: real_stats is missing: the statistics of the real images are not shipped. '
                         f'Pass a dict or the path of a pickle with `mean` and `cov`; the reference opens '
                         f'Evaluation/{want} (Evaluation.calc_inception.Dataset_Statistics computes such a dict)')
    if isinstance(real_stats, (str, os.PathLike)):
        with open(real_stats, 'rb') as f:
            real_stats = pickle.load(f)
    return real_stats['mean'], real_stats['cov']


def Get_Model_FID_Score(generator, load_inception_net=True, device='cuda', gpu_device_ids=None, truncation=1,
                        mean_latent=None, batch_size=100, num_sample=50000, info_print=False, inception=None,
                        real_stats=None):
    """The FID of a generator against `real_stats`, with the reference's signature (gpu_device_ids is accepted and
    unused).  inception: the network with loaded weights; None (with load_inception_net) builds
    load_patched_inception_v3() with its own initialisation."""
    module = getattr(generator, 'module', generator)
    real_mean, real_cov = load_real_stats(real_stats, getattr(module, 'size', None))
    if inception is None:
        if not load_inception_net:
            raise ValueError('Get_Model_FID_Score: load_inception_net=False needs `inception`')
        inception = load_patched_inception_v3().to(device)
    inception.eval()
    stats = Sample_Statistics(generator, inception, truncation, mean_latent, batch_size, num_sample, device,
                              fuse=FID_FUSE, info_print=info_print)
    sample_mean, sample_cov = stats.finish()
    if info_print:
        print('Feature count: ' + str(stats.count) + ' of ' + str(stats.dim))
    return calc_fid(sample_mean, sample_cov, real_mean, real_cov)
