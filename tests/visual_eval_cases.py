"""Cases of the visual-evaluation drivers shared by tools/make_golden_visual_eval.py (reference side) and the tests:
Generator(256, 512, 8), 256^2 inputs from tests/synth.py on both sides.  Fixtures: tests/golden/visual_eval.npz (strided
samples of the float outputs in fp32 and float64, and of the uint8 images) and tests/golden/visual_eval.json (host
selections: seeded picks, file-name pairs, result names, checkpoint keys)."""
import numpy as np
import torch

import synth

VAL_SET_LEN = 3
FWD = dict(tsr_encode='Photo Image', sliced_layer=None, use_tanh=False)
BATCH = dict(name='veval_batch_256', size=256, sets=2, stride=8, **FWD)
VIDEO = dict(name='veval_video_256', size=256, frames=3, stride=8, **FWD)
REL = 5e-5                    # the end-to-end gate of tests/test_reanimate.py (_gate)


def fwd_kwargs(c):
    return {k: c[k] for k in FWD}


def batch_inputs(c=BATCH):
    """The flat eval_img_set: per set one photo and VAL_SET_LEN - 1 renders, each [1,3,256,256], U(-1,1)."""
    out = []
    for s in range(c['sets']):
        out.append(synth.tensor(f"{c['name']}/photo{s}", (1, 3, 256, 256), dist='uniform'))
        out += [synth.tensor(f"{c['name']}/render{s}_{k}", (1, 3, 256, 256), dist='uniform')
                for k in range(VAL_SET_LEN - 1)]
    return out


def video_inputs(c=VIDEO):
    """(photo frames, render frames): lists of [3,256,256] tensors, U(-1,1), as Load_GIF_As_Img_List returns them."""
    p = synth.tensor(c['name'] + '/photo', (c['frames'], 3, 256, 256), dist='uniform')
    r = synth.tensor(c['name'] + '/render', (c['frames'], 3, 256, 256), dist='uniform')
    return list(p), list(r)


def u8_rule_violations(got_u8, ref_u8, ref_float, rel=REL):
    """How many entries break the uint8 rule: an entry may differ from the reference's, by exactly 1, only where the
    reference's float value v puts (clip(v) + 1) * 127.5 within 127.5 * rel * max|image| of an integer; every other
    entry is equal.  got_u8 / ref_u8 [..., H, W, 3] uint8, ref_float [..., 3, H, W] (the same pixels)."""
    v = np.moveaxis(np.asarray(ref_float, dtype=np.float64), -3, -1)
    x = (np.clip(v, -1.0, 1.0) + 1.0) * 127.5
    near = np.abs(x - np.round(x)) <= 127.5 * rel * float(np.abs(v).max())
    diff = np.abs(np.asarray(got_u8).astype(np.int64) - np.asarray(ref_u8).astype(np.int64))
    return int(((diff > 1) | ((diff == 1) & ~near)).sum())


# ------------------------------------------------------------------------------------------------- host selections
PICK_SEED = 11
REAL_FILES, REAL_FACES = 5, 2
SYN_IDS, SYN_FACES = 6, 2
NUM_IMG_PER_ID = 7


def write_real_stacks(directory):
    """REAL_FILES .npy stacks [4 + j, 8, 8, 3] uint8 in `directory`; image k of file j is filled with 10 * j + k, so a
    picked image names its file and position.  Returns the sorted path list."""
    import os
    paths = []
    for j in range(REAL_FILES):
        stack = np.stack([np.full((8, 8, 3), 10 * j + k, np.uint8) for k in range(4 + j)])
        paths.append(os.path.join(str(directory), f'face_{j}.npy'))
        np.save(paths[-1], stack)
    return paths


def id_transform(img):
    return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float()


class SynDataset:
    """(image, render) = constant tensors idx and -idx - 1: a loaded pair names its index."""

    def __len__(self):
        return SYN_IDS * NUM_IMG_PER_ID

    def __getitem__(self, idx):
        idx = int(idx)
        return torch.full((3, 4, 4), float(idx)), torch.full((3, 4, 4), float(-idx - 1))


def picked(tensors):
    """The identifying value of every tensor of a picker's list."""
    return [int(t.reshape(-1)[0].item()) for t in tensors]


def seed_pickers():
    import random
    np.random.seed(PICK_SEED)
    random.seed(PICK_SEED)


SINGLE_FACTOR_FILES = ['anna.png', 'bob.png', 'anna_pose.gif', 'anna_light.gif', 'bob_expression.gif', 'carol_pose.gif',
                       'notes.txt']
VIDEO_FILES = ['frame0.png', 'photo_img.gif', 'render_img.gif']


def touch(directory, names):
    import os
    for n in names:
        open(os.path.join(str(directory), n), 'wb').close()
