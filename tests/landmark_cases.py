"""Cases of the landmark stages (op/landmark.py, Util/landmark_util.py), shared by tools/make_golden_landmark.py, which
records the reference's results in tests/golden/landmark.npz, and by tests/test_landmark.py / test_landmark_gpu.py.
Inputs come from tests/synth.py on both sides; the fixture holds outputs only.

Bounds.  Every value compared against the fixture carries `ref_err`, the reference's own float32 error against the
float64 twin (the tool's restatement of the closed form, which it first asserts equal to the reference in float32), as
tools/make_golden_landmark.py measured and printed it when the fixture was made, and `bound` = 4 * ref_err + one float32
ulp of the value range (`ulp_of`): the two sides differ in association and fma contraction, as GPU and CPU aten do.
Nothing here was derived from the kernels' output.
"""
import numpy as np
import torch
import torch.nn.functional as F

import synth

REFERENCE_SCALE = 195.0          # SFDDetector.reference_scale
FALLBACK_BBOX = [0, 0, 255, 255, 1]


def ulp_of(value_range):
    """One float32 ulp at |value_range|."""
    return float(np.spacing(np.float32(abs(value_range))))


def bound(ref_err, value_range, margin=4.0):
    return margin * ref_err + ulp_of(value_range)


# ----------------------------------------------------------------------------- crop
# center / scale per sample go through transform() to the boxes (ux, uy, bx, by) written beside them: the tool asserts that
# its transform gives them, the tests that Face_Crop_Boxes does.
CROP_CASES = {
    # [3, 3, 48, 40] images (not square: an x / y swap shows), 32 x 32 crops:
    #   sample 0  a box inside the image, 22 x 21 (Hc != Wc): upsampling
    #   sample 1  53 x 53, beyond all four edges
    #   sample 2  100 x 100 canvas: more than 2 x R, source pixels are skipped; beyond all four edges too
    'crop_small': dict(shape=(3, 3, 48, 40), r=32,
                       center=[(20.2, 24.6), (19.5, 24.3), (25.3, 20.7)], scale=[0.11, 0.28, 0.52],
                       box=[(9, 14, 31, 35), (-6, -1, 47, 52), (-23, -28, 77, 72)],
                       # measured by the tool: reference fp32 against the float64 twin; bounds 5.19e-07 forward, 9.43e-07
                       # backward
                       fwd_ref_err=1.149e-07, fwd_range=9.731e-01, bwd_ref_err=2.060e-07, bwd_range=1.993e+00, stride=1),
    # [2, 3, 256, 256] images, 256 x 256 crops, the detector's fallback box: a 520 x 520 canvas, down by 2.03.  The fixture
    # keeps every 9th row and column of the output and of the gradient (the whole tensors are 1.5 MB each).  Bounds
    # 6.19e-07 forward, 6.86e-07 backward.
    'crop_fallback': dict(shape=(2, 3, 256, 256), r=256, bbox=[FALLBACK_BBOX, FALLBACK_BBOX],
                          box=[(-131, -162, 389, 358), (-131, -162, 389, 358)],
                          fwd_ref_err=1.400e-07, fwd_range=9.873e-01, bwd_ref_err=1.416e-07, bwd_range=1.674e+00, stride=9),
}


def crop_image(name):
    return synth.tensor(f'landmark/{name}/img', CROP_CASES[name]['shape'], dist='uniform')


def crop_grad(name):
    c = CROP_CASES[name]
    return synth.tensor(f'landmark/{name}/go', (c['shape'][0], 3, c['r'], c['r']))


def box_center_scale(bbox):
    """Crop_An_Image's arithmetic for a bounding box of plain numbers."""
    center = torch.tensor([bbox[2] - (bbox[2] - bbox[0]) / 2.0, bbox[3] - (bbox[3] - bbox[1]) / 2.0])
    center[1] = center[1] - (bbox[3] - bbox[1]) * 0.12
    return center, (bbox[2] - bbox[0] + bbox[3] - bbox[1]) / REFERENCE_SCALE


def crop_center_scale(name):
    """(center_list, scale_list) of a crop case: written out, or from its bounding boxes."""
    c = CROP_CASES[name]
    if 'bbox' in c:
        pairs = [box_center_scale(b) for b in c['bbox']]
        return [p[0] for p in pairs], [p[1] for p in pairs]
    return [torch.tensor(p, dtype=torch.float32) for p in c['center']], list(c['scale'])


# ----------------------------------------------------------------------------- decode
DECODE_VALUE = 2.0               # the planted maximum; the background is 0.1 * N(0, 1)
# (row, column) of the maximum of each of the ten maps of a case ([2, 5, 64, 64]: map = sample * 5 + channel), and for the
# interior ones the signs of right - left and below - above ('+', '-', '0': equal neighbours).
DECODE_CASES = {
    # the four corners, the four edges (no offset applies; the bottom edge and corners are last-row maxima), an exact
    # tie (the first flat index wins: its lane in the kernel's wave is the higher one), the last row again
    'decode_border': dict(cs_seed=0, maps=[
        dict(at=(0, 0)), dict(at=(0, 63)), dict(at=(63, 0)), dict(at=(63, 63)),
        dict(at=(0, 17)), dict(at=(63, 40)), dict(at=(29, 0)), dict(at=(33, 63)),
        dict(at=(10, 40), tie=(30, 8), signs='+-'), dict(at=(63, 1))]),
    # every sign pattern of an interior maximum, and one map with no planted value at all
    'decode_interior': dict(cs_seed=0, maps=[
        dict(at=(5, 9), signs='++'), dict(at=(20, 31), signs='+-'), dict(at=(31, 20), signs='-+'),
        dict(at=(62, 62), signs='--'), dict(at=(1, 1), signs='00'), dict(at=(40, 7), signs='0+'),
        dict(at=(7, 40), signs='-0'), dict(at=(50, 50), signs='+0'), dict(at=(13, 60), signs='0-'), dict()]),
}
_NEIGHBOURS = {'+': (1.0, 0.5), '-': (0.5, 1.0), '0': (0.75, 0.75)}      # (right or below, left or above)


def decode_maps(name):
    """hm [2, 5, 64, 64] float32 of a decode case."""
    hm = synth.tensor(f'landmark/{name}/hm', (2, 5, 64, 64), scale=0.1)
    for m, spec in enumerate(DECODE_CASES[name]['maps']):
        plane = hm[m // 5, m % 5]
        if 'at' not in spec:
            continue
        y, x = spec['at']
        plane[y, x] = DECODE_VALUE
        if 'signs' in spec:
            (r, l), (b, a) = _NEIGHBOURS[spec['signs'][0]], _NEIGHBOURS[spec['signs'][1]]
            plane[y, x + 1], plane[y, x - 1], plane[y + 1, x], plane[y - 1, x] = r, l, b, a
        if 'tie' in spec:
            plane[spec['tie'][0], spec['tie'][1]] = DECODE_VALUE
    return hm


def decode_center_scale(name, seed=None):
    """(center [2, 2], scale [2]) float32 of a decode case; the tool picks the case's cs_seed so that no preds_orig value
    lies within 1e-3 of an integer before its truncation."""
    seed = DECODE_CASES[name]['cs_seed'] if seed is None else seed
    center = synth.tensor(f'landmark/{name}/center', (2, 2), seed=seed, dist='uniform', scale=60.0, shift=128.0)
    scale = synth.tensor(f'landmark/{name}/scale', (2,), seed=seed, dist='uniform', scale=0.8, shift=1.6)
    return center, scale


def decode_expected_preds(name):
    """preds [2, 5, 2] of a decode case from its table alone (the maps without a planted value: None)."""
    out = []
    for spec in DECODE_CASES[name]['maps']:
        if 'at' not in spec:
            out.append(None)
            continue
        y, x = spec['at']
        dx, dy = ({'+': 0.25, '-': -0.25, '0': 0.0}[s] for s in spec.get('signs', '00'))
        out.append((x + 1 + dx - 0.5, y + 1 + dy - 0.5))
    return out


# ----------------------------------------------------------------------------- distance
# bounds: 5.27e-04 on the sums (values up to 2980: two ulps), 1.05e-06 on the gradients
DISTANCE_CASE = dict(shape=(3, 4, 64, 64), out_ref_err=7.081e-05, out_range=2.980e+03, grad_ref_err=2.034e-07,
                     grad_range=2.730e+00, stride=4)


def distance_inputs():
    shape = DISTANCE_CASE['shape']
    return (synth.tensor('landmark/dist/a', shape, scale=0.3), synth.tensor('landmark/dist/b', shape, scale=0.3),
            synth.tensor('landmark/dist/g', (shape[0],)))


# ----------------------------------------------------------------------------- end to end: stand-in networks
E2E = dict(shape=(3, 3, 64, 56), shifts=(0.2, -0.6, 0.8), maps=3, hm_stride=2,
           # sample 0: its own box; sample 1: filtered out (score below 1/2); sample 2: a box that leaves [0, 255].
           # Bounds: 3.48e-07 on the heat maps, 1.11e-07 on the loss, 2.75e-08 on its gradient.
           bbox=[[17, 16, 51, 49, None], FALLBACK_BBOX, FALLBACK_BBOX],
           hm_ref_err=7.963e-08, hm_range=3.222e-01, loss_ref_err=1.289e-08, loss_range=5.153e-01,
           grad_ref_err=6.758e-09, grad_range=6.293e-03)


def e2e_images(which):
    """`which` in ('g', 'r'): [3, 3, 64, 56] in [-1, 1], one brightness per sample (what the stand-in detector reads)."""
    noise = synth.tensor(f'landmark/e2e/{which}', E2E['shape'], dist='uniform', scale=0.2)
    shift = torch.tensor(E2E['shifts'], dtype=torch.float32).view(-1, 1, 1, 1)
    return noise + shift


class DetectorNet(torch.nn.Module):
    """Stand-in for the SFD network: one (class, regression) pair of maps from 8 x 8 means of its input."""

    def __init__(self):
        super().__init__()
        self.cls = torch.nn.Parameter(torch.tensor([[0., 0., 0.], [1., 1., 1.]]).view(2, 3, 1, 1) / 100)
        self.reg = torch.nn.Parameter(torch.tensor([[1., 1., 1.], [1., -1., .5], [1., 1., 1.], [-.5, 1., .2]])
                                      .view(4, 3, 1, 1) / 300)

    def forward(self, x):
        pooled = F.avg_pool2d(x, 8)
        return [F.conv2d(pooled, self.cls), F.conv2d(pooled, self.reg)]


def standin_get_predictions(olist, batch_size=1):
    """Stand-in for face_alignment.detection.sfd.detect.get_predictions: one box from the means of the two maps, its
    corners rounded to whole pixels; a bright image gets a box that starts left of 0."""
    cls, reg = olist
    score = float(cls[0, 1].mean())
    t = np.tanh(reg[0].reshape(4, -1).mean(1).astype(np.float64))
    cx, cy, hw, hh = 30 + 10 * t[0], 32 + 10 * t[1], 14 + 8 * t[2], 16 + 8 * t[3]
    x0 = cx - hw - 4000 * max(0.0, t[0] - 0.7)
    box = np.rint([x0, cy - hh, cx + hw, cy + hh])
    return [np.array([list(box) + [score]], dtype=np.float32)]


class Detector:
    reference_scale = REFERENCE_SCALE

    def __init__(self, net):
        self.face_detector = net

    @staticmethod
    def _filter_bboxes(bboxlist):
        return [b for b in bboxlist if b[-1] > 0.5]


class AlignmentNet(torch.nn.Sequential):
    """Stand-in for the FAN: two stride-2 convolutions, [N, 3, 256, 256] -> [N, maps, 64, 64]."""

    def __init__(self, maps=E2E['maps']):
        super().__init__(torch.nn.Conv2d(3, 8, 4, 2, 1), torch.nn.ReLU(), torch.nn.Conv2d(8, maps, 4, 2, 1))
        sd = {k: synth.tensor(f'landmark/fan/{k}', v.shape, scale=(0.5 / max(v[0].numel(), 1) ** 0.5 if v.ndim == 4 else 0.1))
              for k, v in self.state_dict().items()}
        self.load_state_dict(sd)


class Alignment:
    """What the stages read of a face_alignment.FaceAlignment."""

    def __init__(self, device='cpu', dtype=torch.float32):
        self.face_detector = Detector(DetectorNet().to(device=device, dtype=dtype).requires_grad_(False).eval())
        self.face_alignment_net = AlignmentNet().to(device=device, dtype=dtype).requires_grad_(False).eval()


def stub_modules(transform=None, get_preds_fromhm=None):
    """{module name: module} of a stand-in `face_alignment` package for sys.modules: get_predictions above, and for the
    reference's import also `transform` / `get_preds_fromhm` of face_alignment.utils."""
    import types
    mods = {n: types.ModuleType(n) for n in ('face_alignment', 'face_alignment.detection', 'face_alignment.detection.sfd',
                                             'face_alignment.detection.sfd.detect', 'face_alignment.utils')}
    mods['face_alignment.detection.sfd.detect'].get_predictions = standin_get_predictions
    mods['face_alignment.utils'].transform = transform
    mods['face_alignment.utils'].get_preds_fromhm = get_preds_fromhm
    mods['face_alignment'].detection = mods['face_alignment.detection']
    mods['face_alignment'].utils = mods['face_alignment.utils']
    mods['face_alignment.detection'].sfd = mods['face_alignment.detection.sfd']
    mods['face_alignment.detection.sfd'].detect = mods['face_alignment.detection.sfd.detect']
    return mods
