"""Dual-supervision (disentanglement) iteration cases, shared by tools/make_golden_ds.py (reference side) and the tests.

A dual-supervision batch pairs each photo with its partner's render (dataset.py:361-406); the G step then adds the
face-regional loss (Util/training_util.py:228-256) on the region where the render is not background.  Synthetic
renders here are built so that this region is decided identically in every precision: the background is exactly -1
in every channel (mean exactly -1, "> -1" is false), and the face region's values lie in [-0.5, 1] (mean far from -1).
"""
import numpy as np
import torch

import synth

# train_3_encoder_hyperparams.py:49-50, 66-71
DS_HP = dict(ds_freq=2, ex_ds_freq=3, rec_face_reg_loss_lambda=0, ds_face_reg_loss_lambda=20,
             ep_face_reg_loss_lambda=100, ep_lpips_l1_weight_shrink=10)

# The G phase of one dual-supervision batch and of one extreme-pose batch: Generator(256) (the term needs render size =
# output size), n_mlp=2, Discriminator(256) as D (seed 8) and a second Discriminator(256) as D_edit (seed 10), B=4.
DS_CASE = dict(name='train_ds_256', size=256, b=4, n_mlp=2, d_seed=8, d_edit_seed=10)
DS_PHASES = ('ds', 'ep')


def face_render(name, shape, seed=0):
    """Deterministic render [N, C, H, W]: an ellipse per sample (centre and radii vary with the sample) holding values
    in [-0.5, 1], exactly -1 everywhere else."""
    n, c, h, w = (int(s) for s in shape)
    vals = synth.tensor(name + '/vals', (n, c, h, w), seed=seed, dist='uniform', scale=0.75, shift=0.25)
    geo = synth.tensor(name + '/geo', (n, 4), seed=seed, dist='uniform').double()
    yy = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    xx = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    cy = (0.5 + 0.08 * geo[:, 0]).view(n, 1, 1) * h
    cx = (0.5 + 0.08 * geo[:, 1]).view(n, 1, 1) * w
    ry = (0.38 + 0.06 * geo[:, 2]).view(n, 1, 1) * h
    rx = (0.30 + 0.06 * geo[:, 3]).view(n, 1, 1) * w
    inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    out = torch.full((n, c, h, w), -1.0, dtype=torch.float32)
    return torch.where(inside.unsqueeze(1), vals, out).contiguous()


def loader_batch(c, phase):
    """(photo, render) as a loader yields them for this phase's batch, before Data_Loading pairs them."""
    key = f"{c['name']}/{phase}"
    photo = synth.tensor(key + '/photo', (c['b'], 3, 256, 256), dist='uniform')
    render = face_render(key + '/render', (c['b'], 3, 256, 256))
    return photo, render


def paired(photo, render, extreme):
    """Data_Loading's dual-supervision pairing (dataset.py:343-406): render and target of the partner image; extreme
    pose keeps the even members.  Returns (g_input, r_input, g_ref)."""
    idx = np.arange(photo.shape[0]) ^ 1
    g_input, r_input, g_ref = photo, render[idx], photo[idx]
    if extreme:
        g_input, r_input, g_ref = g_input[0::2], r_input[0::2], g_ref[0::2]
    return g_input, r_input, g_ref


def face_lambda(ds_flag, extreme_ds_flag, hp=DS_HP):
    """Weight of the face-regional term (train_3_encoder.py:521-526)."""
    if not ds_flag:
        return hp['rec_face_reg_loss_lambda']
    return hp['ep_face_reg_loss_lambda'] if extreme_ds_flag else hp['ds_face_reg_loss_lambda']


def ds_flags_reference(n_iter, ds_freq, ex_ds_freq):
    """The reference loop's flag sequence (train_3_encoder.py:780-786), restated: [(ds_flag, extreme_ds_flag), ...]."""
    out, ds_count = [], 0
    for iter_idx in range(n_iter):
        if (iter_idx % ds_freq) == (ds_freq - 1):
            ds_flag = True
            extreme = (ds_count % ex_ds_freq) == (ex_ds_freq - 1)
            ds_count += 1
        else:
            ds_flag, extreme = False, False
        out.append((ds_flag, extreme))
    return out


def pack(flat):
    """Gradient samples of a fixture, one zip member per (phase, network, field) instead of one per tensor: '<p>/<net>/
    <name>/<field>' entries (tests/cases.py::grad_sample's s / n / s64 / n64) -> '<p>/<net>/@names', '@<field>' (the
    samples concatenated) and '@<field>_off' (offsets).  Other entries pass through."""
    out, groups = {}, {}
    for key, v in flat.items():
        parts = key.split('/')
        if len(parts) >= 4 and parts[-1] in ('s', 'n', 's64', 'n64'):
            groups.setdefault('/'.join(parts[:2]), {}).setdefault('/'.join(parts[2:-1]), {})[parts[-1]] = v
        else:
            out[key] = v
    for pre, tensors in groups.items():
        names = sorted(tensors)
        out[pre + '/@names'] = np.array(names)
        for field in ('s', 's64'):
            arrs = [np.asarray(tensors[n][field]).reshape(-1) for n in names]
            out[f'{pre}/@{field}'] = np.concatenate(arrs)
            out[f'{pre}/@{field}_off'] = np.cumsum([0] + [len(a) for a in arrs]).astype(np.int64)
        for field in ('n', 'n64'):
            out[f'{pre}/@{field}'] = np.array([tensors[n][field] for n in names], dtype=np.float64)
    return out


class Unpacked:
    """Inverse of pack(): a read-only mapping with `.files`, like the NpzFile tests/test_hip_train.py::check_grads reads."""

    def __init__(self, npz):
        raw = {k: npz[k] for k in npz.files}       # an NpzFile decompresses a member on every access
        self._d = {k: v for k, v in raw.items() if '/@' not in k}
        for key in raw:
            if not key.endswith('/@names'):
                continue
            pre = key[:-len('/@names')]
            for i, name in enumerate(raw[key]):
                for field in ('s', 's64'):
                    off = raw[f'{pre}/@{field}_off']
                    self._d[f'{pre}/{name}/{field}'] = raw[f'{pre}/@{field}'][off[i]:off[i + 1]]
                for field in ('n', 'n64'):
                    self._d[f'{pre}/{name}/{field}'] = raw[f'{pre}/@{field}'][i]
        self.files = list(self._d)

    def __getitem__(self, key):
        return self._d[key]
