"""FID cases shared by tools/make_golden_fid.py (reference side) and the tests.  Fixture: tests/golden/fid.npz, outputs
only: per case `/fid` (the reference's calc_fid), and the reference's own spread, which is the tests' tolerance:
    `/spread_sym`   |FID_ref(a, b) - FID_ref(b, a)|                        FID is symmetric in its two arguments
    `/spread_mean`  |FID_ref(float32 means) - FID_ref(float64 means)|      the reference's np.mean of fp32 features is fp32
`tolerance(golden, name)` is 10 x the larger of the two: two samples understate a tail, and one order of magnitude is still
many orders below any difference that matters in an FID.

CALC_CASES (name, D, N1, N2): the reference's calc_fid on np.mean / np.cov of the relu-like fp32 `features` below, which
have a non-zero mean.  `rank` has fewer samples than features: both covariances are rank-deficient.
SAMPLE_CASES: the reference's extract_feature_from_samples -> np.mean / np.cov -> calc_fid against `real_stats()`, with
fixed latents (`latents`: the stand-in for torch.randn on the reference side, the `sampler` on ours), n_sample = 70 at
batch_size = 32: batches of 32 and 38.  `toy`: a small generator that also runs on the CPU; `g64`: the project's / the
reference's Generator(64) with tests/synth.py's weights and the stored noise pinned.  Both use StandinInception (64
features).  Inputs and weights come from tests/synth.py on both sides.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import synth

CALC_CASES = [('d64', 64, 200, 207), ('d128', 128, 1000, 1007), ('rank', 128, 96, 103)]
SAMPLE_CASES = [dict(name='toy', kind='toy', n_sample=70, batch=32), dict(name='g64', kind='generator', size=64,
                                                                           n_sample=70, batch=32)]
SAMPLE_BY_NAME = {c['name']: c for c in SAMPLE_CASES}
FEATURES = 64               # of the stand-in inception


def features(name, which, n, d):
    """[n, d] fp32 numpy: relu of correlated Gaussians with a bias; set 'b' is shifted and scaled against set 'a'."""
    z = synth.tensor(f'fid/{name}/{which}/z', (n, d))
    mix = synth.tensor(f'fid/{name}/mix', (d, d), scale=(1.0 / d) ** 0.5)
    bias = synth.tensor(f'fid/{name}/bias', (d,), scale=0.3, shift=0.5)
    gain = 1.0 if which == 'a' else 1.15
    return torch.relu(gain * (z @ mix) + bias + (0.0 if which == 'a' else 0.1)).numpy()


def moments(feat):
    """(mean, cov) as the reference takes them: np.mean keeps the features' dtype, np.cov is float64."""
    return np.mean(feat, 0), np.cov(feat, rowvar=False)


def real_stats():
    """The `real` statistics of the sample cases: those of 207 relu-like features, float64."""
    feat = features('real', 'b', 207, FEATURES).astype(np.float64)
    mean, cov = moments(feat)
    return {'mean': mean, 'cov': cov}


def latents(c, batch_index, batch):
    """z [batch, 512] of one batch, fp32 on the CPU."""
    return synth.tensor(f"fid/{c['name']}/z/{batch_index}", (batch, 512))


def sampler(c):
    """The `sampler` argument of Evaluation.fid.Sample_Statistics for case c."""
    def sample(batch_index, batch, latent_dim, device):
        assert latent_dim == 512
        return latents(c, batch_index, batch).to(device)
    return sample


def tolerance(golden, name):
    return 10 * max(float(golden[name + '/spread_sym']), float(golden[name + '/spread_mean']))


U = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u) in float64: the relative error bound of a sum of k terms in any order."""
    return k * U / (1 - k * U)


def moment_bounds(feat, shift):
    """(mean bound [D], cov bound [D, D]) on |Feature_Statistics - np.mean / np.cov| for the float64 features `feat`
    [n, D] and the state's shift, from the data.  With y = feat - shift, s = sum_b y:
      * either side's second moment is a sum of n products (plus the rounding of each centred value and of each product:
        n + 2 terms' worth), whatever the order: error <= gamma_(n+2) * sum_b |y_bi y_bj| for the shifted form, and the
        same expression bounds np.cov's centred sum, because sum_b |z_bi z_bj| <= sum_b |y_bi y_bj| + |s_i s_j| / n * 3
        for z = y - s / n (expand and apply |s_i| <= sum_b |y_bi|);
      * the correction s_i s_j / n carries the two sums' errors: 2 gamma_(n+2) * (sum_b |y_bi|)(sum_b |y_bj|) / n;
      * both sides, and the final division: a factor 2 and gamma_(n+2) -> gamma_(n+4).
    mean: shift + s / n against np.mean: 2 * gamma_(n+2) * (|shift| + sum_b |y_b| / n)."""
    n = feat.shape[0]
    y = feat - shift
    ay = np.abs(y)
    s1 = ay.sum(0)
    second = ay.T @ ay + 5 * np.outer(s1, s1) / n
    return 2 * gamma(n + 2) * (np.abs(shift) + s1 / n), 2 * gamma(n + 4) * second / (n - 1)


def _synth_weights(module, prefix):
    sd = {}
    for k, v in module.state_dict().items():
        scale = 0.1 if v.ndim == 1 else (1.0 / v.shape[1]) ** 0.5
        sd[k] = synth.tensor(prefix + k, v.shape, scale=scale)
    module.load_state_dict(sd)
    return module.eval().requires_grad_(False)


class ToyGenerator(nn.Module):
    """z [B, 512] -> tanh image [B, 3, 16, 16]; takes the call of the reference's FID loop."""
    size = 16

    def __init__(self):
        super().__init__()
        self.style = nn.Sequential(nn.Linear(512, 32), nn.LeakyReLU(0.2))
        self.to_image = nn.Linear(32, 3 * 16 * 16)
        _synth_weights(self, 'fid/toy_generator/')

    def forward(self, styles, truncation=1, truncation_latent=None):
        assert len(styles) == 1 and truncation == 1
        return torch.tanh(self.to_image(self.style(styles[0]))).view(-1, 3, 16, 16)


class Pinned(nn.Module):
    """A Generator with the stored noise pinned (the FID loop passes none, and fresh noise cannot be compared)."""

    def __init__(self, g):
        super().__init__()
        self.g, self.size = g, g.size

    def forward(self, styles, **kw):
        return self.g(styles, randomize_noise=False, **kw)


class StandinInception(nn.Module):
    """[B, 3, S, S] -> [[B, 64, 1, 1]]: a 4 x 4 average pool, a linear map and a relu with a positive bias."""

    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(3 * 4 * 4, FEATURES)
        _synth_weights(self, 'fid/standin_inception/')

    def forward(self, img):
        pooled = F.adaptive_avg_pool2d(img, 4).flatten(1)
        return [torch.relu(3.0 * self.fc(pooled) + 0.5).view(img.shape[0], FEATURES, 1, 1)]
