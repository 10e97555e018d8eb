"""Running mean and covariance of the FID's Inception features (reference Evaluation/fid.py:126-127 and
calc_inception.py:118-119: np.mean / np.cov over all features on the host, at the end).

The reference copies every batch's [B, 2048] features to the host (a synchronisation per batch), concatenates them and
runs np.cov over [50000, 2048] in float64.  Feature_Statistics keeps shifted first and second moments on the device, in
float64, and adds a batch to them with one HIP launch (csrc/fid_stats.hip, the fp64 matrix instruction):

    y      = float64(feat) - shift            shift [D]: fixed before the first update (default: the first batch's mean)
    sum   += sum_b y                          [D]
    outer += sum_b y_i y_j   for i <= j       [D, D]; elements below the diagonal are not meaningful
    count += B                                a Python int: batch sizes are known without a synchronisation

    mean = shift + sum / n                    cov_ij = cov_ji = (outer_ij - sum_i sum_j / n) / (n - 1)

The shift keeps the subtraction in cov free of cancellation (relu features have means of the size of their deviations);
with it the result is np.cov's to float64 rounding.  merge() re-centres another state to this one's shift exactly (float64
algebra, no samples needed): how the states of several processes, one per GPU, are combined.

The composite path is the same formulas in float64 torch ops (addmm_): CPU tensors, other dtypes, D % 16 != 0, fuse=False.
"""
import torch

from . import _native


def _mirror(outer):
    """The full symmetric matrix from the meaningful upper triangle."""
    upper = torch.triu(outer)
    return upper + torch.triu(outer, 1).T


class Feature_Statistics:
    def __init__(self, dim, device, shift=None, fuse=True):
        self.dim, self.device, self.fuse = int(dim), torch.device(device), bool(fuse)
        self.count = 0
        self.shift = None if shift is None else torch.as_tensor(shift).to(self.device, torch.float64).reshape(dim).clone()
        self.sum = torch.zeros((self.dim,), dtype=torch.float64, device=self.device)
        self.outer = torch.zeros((self.dim, self.dim), dtype=torch.float64, device=self.device)

    def _fused(self, feat):
        return self.fuse and feat.is_cuda and feat.dtype == torch.float32 and self.sum.is_cuda and \
            _native.fid_stats_serves(feat.shape[0], self.dim)

    def update(self, feat):
        """Adds the rows of feat [B, D] (on the state's device).  Nothing synchronises."""
        if feat.ndim != 2 or feat.shape[1] != self.dim:
            raise ValueError(f'Feature_Statistics.update: features {tuple(feat.shape)}, expected [B, {self.dim}]')
        if feat.shape[0] == 0:
            return self
        with torch.no_grad():
            feat = feat.detach().to(self.device)
            if self.shift is None:
                self.shift = feat.to(torch.float64).mean(0)
            if not (self._fused(feat) and _native.fid_stats_update(feat.contiguous(), self.shift, self.sum, self.outer)):
                y = feat.to(torch.float64) - self.shift
                self.sum += y.sum(0)
                self.outer.addmm_(y.T, y)
            self.count += feat.shape[0]
        return self

    def finish(self):
        """(mean [D], cov [D, D]) as float64 tensors on the state's device; cov is exactly symmetric."""
        n = self.count
        if n < 2:
            raise ValueError(f'Feature_Statistics.finish: {n} samples: a covariance needs two')
        if self.fuse and self.sum.is_cuda:
            return _native.fid_stats_finish(self.sum, self.outer, self.shift, n)
        with torch.no_grad():
            mean = self.shift + self.sum / n
            cov = torch.triu((self.outer - (self.sum[:, None] * self.sum[None, :]) / n) / (n - 1))
            return mean, cov + torch.triu(cov, 1).T

    def merge(self, other):
        """Adds another state's samples, re-centred to this state's shift: with delta = other.shift - shift every sample
        of `other` is y + delta here, so sum' = sum_o + n_o delta and outer' = outer_o + delta sum_o^T + sum_o delta^T +
        n_o delta delta^T, exactly (float64 torch ops)."""
        if other.dim != self.dim:
            raise ValueError(f'Feature_Statistics.merge: {other.dim} features into {self.dim}')
        if other.count == 0:
            return self
        with torch.no_grad():
            o_shift, o_sum, o_outer = (t.to(self.device) for t in (other.shift, other.sum, other.outer))
            if self.shift is None:
                self.shift = o_shift.clone()
            delta = o_shift - self.shift
            n = other.count
            self.sum += o_sum + n * delta
            cross = delta[:, None] * o_sum[None, :]
            self.outer += _mirror(o_outer) + cross + cross.T + n * (delta[:, None] * delta[None, :])
            self.count += n
        return self
