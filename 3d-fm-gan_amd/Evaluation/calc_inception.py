"""Inception features and statistics of a dataset (reference Evaluation/calc_inception.py:59-81 and the np.mean / np.cov
of its script half, :118-124).

    load_patched_inception_v3   :59-65    InceptionV3([3], normalize_input=False); `weights` is the published FID
                                          checkpoint's state dict (None: own initialisation, a load figure)
    extract_features            :68-81    every batch's features, on the CPU, concatenated (the reference's signature;
                                          one transfer per batch, kept for parity)
    Dataset_Statistics                    {'mean', 'cov'} as float64 numpy, the fields of the statistics pickle, through
                                          op.fid_stats.Feature_Statistics: nothing leaves the device inside the loop

Out of scope: the lmdb dataset and the command line of the reference's script half.
"""
import torch

from op.fid_stats import Feature_Statistics

from .inception import InceptionV3


def load_patched_inception_v3(weights=None):
    return InceptionV3([3], normalize_input=False, weights=weights)


def features_of(inception, img, fuse=True):
    """[B, D] features of one image batch: the network's first output, flattened.  `fuse` reaches an InceptionV3's input
    stage; any other callable is called as the reference calls it."""
    out = inception(img, fuse=fuse) if isinstance(inception, InceptionV3) else inception(img)
    return out[0].reshape(img.shape[0], -1)


@torch.no_grad()
def extract_features(loader, inception, device):
    feature_list = []
    for img in loader:
        img = img.to(device)
        feature_list.append(features_of(inception, img).to('cpu'))
    return torch.cat(feature_list, 0)


@torch.no_grad()
def Dataset_Statistics(loader, inception, device, fuse=True):
    """{'mean': [D], 'cov': [D, D]} float64 numpy arrays of the features of every image the loader yields."""
    stats = None
    for img in loader:
        feat = features_of(inception, img.to(device), fuse)
        if stats is None:
            stats = Feature_Statistics(feat.shape[1], feat.device, fuse=fuse)
        stats.update(feat)
    if stats is None:
        raise ValueError('Dataset_Statistics: the loader yielded no batch')
    mean, cov = stats.finish()
    return {'mean': mean.cpu().numpy(), 'cov': cov.cpu().numpy()}
