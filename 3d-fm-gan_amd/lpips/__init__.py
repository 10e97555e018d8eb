"""LPIPS perceptual loss, `net-lin` / VGG16 form — the term `lpips_loss_lambda * LPIPS_Loss(g_output, g_ref, lpips_model)`
of the reference's G step (train_3_encoder.py:373-374,529; Util/training_util.py:115-127).

Topology restated from lpips/networks_basic.py:36-121 (PNetLin: ScalingLayer -> VGG16 features cut after relu1_2,
relu2_2, relu3_3, relu4_3, relu5_3 (lpips/pretrained_networks.py:106-141) -> unit-normalise over channels -> squared
difference -> 1x1 conv to one channel -> spatial mean -> sum over the five taps) and lpips/__init__.py:22-53
(PerceptualLoss.forward(pred, target) evaluates net(target, pred)).

Weights: the reference downloads torchvision's ImageNet VGG16 and ships `weights/v0.1/vgg.pth` for the 1x1 layers; neither
is available offline, and the reference's module itself is not importable here (it needs torchvision,
skimage, IPython).  So this module is **load, not a parity row**: same layers, same tensor shapes, same arithmetic per
layer, random initialisation unless `load_state_dict` is given real weights (state_dict names follow the reference:
`net.slice1.0.weight` ... `lin4.model.1.weight`, `scaling_layer.shift/scale`).  It is frozen and in eval mode in the
training step, so only data gradients flow through it.

The VGG trunk is host PyTorch-ROCm (MIOpen convs).  The distance behind each tap (normalise, difference, square, 1x1
conv, spatial mean) runs on the kernel of op/lpips_distance.py (csrc/lpips_distance.hip) when the module is in eval mode
(dropout inactive) and the features are float32, NHWC-dense CUDA tensors with autocast off; otherwise (CPU tensors,
bf16 features of the autocast leg, NCHW features, training mode) it is the aten composite below, as before.  Switch:
`lpips.FUSED` (environment FMGAN_LPIPS_FUSED, default 1).
"""
import os

import torch
from torch import nn

from op.lpips_distance import lpips_distance, lpips_distance_serves

# Per-tap distance on the HIP kernel where it serves; False keeps the aten composite everywhere.
FUSED = os.environ.get('FMGAN_LPIPS_FUSED', '1') != '0'

# VGG16 `features` indices -> (slice, [(index, cin, cout) convs]); a MaxPool2d(2) opens slices 2..5
_VGG_SLICES = (
    ((0, 3, 64), (2, 64, 64)),
    ((5, 64, 128), (7, 128, 128)),
    ((10, 128, 256), (12, 256, 256), (14, 256, 256)),
    ((17, 256, 512), (19, 512, 512), (21, 512, 512)),
    ((24, 512, 512), (26, 512, 512), (28, 512, 512)),
)


class vgg16(nn.Module):
    """VGG16 conv trunk in five slices; module indices inside a slice are torchvision's `features` indices."""

    def __init__(self, requires_grad=False):
        super().__init__()
        self.N_slices = 5
        for si, convs in enumerate(_VGG_SLICES):
            seq = nn.Sequential()
            if si > 0:
                seq.add_module(str(convs[0][0] - 1), nn.MaxPool2d(kernel_size=2, stride=2))
            for idx, cin, cout in convs:
                seq.add_module(str(idx), nn.Conv2d(cin, cout, kernel_size=3, padding=1))
                seq.add_module(str(idx + 1), nn.ReLU(inplace=True))
            setattr(self, f'slice{si + 1}', seq)
        if not requires_grad:
            self.requires_grad_(False)

    def forward(self, x):
        taps = []
        for si in range(5):
            x = getattr(self, f'slice{si + 1}')(x)
            taps.append(x)
        return taps


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('scale', torch.tensor([.458, .448, .450])[None, :, None, None])

    def forward(self, inp):
        return (inp - self.shift) / self.scale


class NetLinLayer(nn.Module):
    """Dropout (inactive in eval mode) + 1x1 conv without bias, non-negative weights (the reference clamps them)."""

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers.append(nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False))
        self.model = nn.Sequential(*layers)
        with torch.no_grad():
            self.model[-1].weight.abs_()


def normalize_tensor(in_feat, eps=1e-10):
    return in_feat / (torch.sqrt(torch.sum(in_feat ** 2, dim=1, keepdim=True)) + eps)


class PNetLin(nn.Module):
    chns = (64, 128, 256, 512, 512)

    def __init__(self, use_dropout=True):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.net = vgg16(requires_grad=False)
        for i, c in enumerate(self.chns):
            setattr(self, f'lin{i}', NetLinLayer(c, use_dropout=use_dropout))

    def forward(self, in0, in1):
        s0 = self.scaling_layer(in0)
        return self.forward_scaled(s0, s0 if in1 is in0 else self.scaling_layer(in1))

    def forward_scaled(self, s0, s1):
        """The trunk and the distances on inputs that already went through the ScalingLayer (op/ppl_input.py produces
        them in one launch)."""
        # MIOpen's convolutions are not bit-reproducible from call to call (two trunk passes over the same values differ
        # in the last bit at every tap), so the distance of an image to itself is exactly 0 only if its features are
        # computed once.
        f0 = self.net(s0)
        return self._tap_sum(f0, f0 if s1 is s0 else self.net(s1))

    def features_scaled(self, s):
        """The five trunk taps of an input that already went through the ScalingLayer: what forward_scaled computes for
        each side, to be kept when one side never changes (the target of an image projection)."""
        return self.net(s)

    def forward_features(self, f0, s1):
        """forward_scaled(s0, s1) with the trunk pass over s0 already done: f0 = features_scaled(s0)."""
        return self._tap_sum(f0, self.net(s1))

    def _tap_sum(self, f0, f1):
        """The distance from the two lists of trunk taps: per tap the kernel where it serves, else the composite; the
        taps added in order."""
        val = None
        for i in range(len(self.chns)):
            lin = getattr(self, f'lin{i}').model
            if FUSED and not self.training and lpips_distance_serves(f0[i], f1[i], lin[-1].weight):
                r = lpips_distance(f0[i], f1[i], lin[-1].weight)
            else:
                diff = (normalize_tensor(f0[i]) - normalize_tensor(f1[i])) ** 2
                r = lin(diff).mean([2, 3], keepdim=True)
            val = r if val is None else val + r
        return val


def scaling_layer_of(percept, method):
    """percept's ScalingLayer when a caller may scale the inputs itself and hand them to `method` (forward_scaled,
    forward_cached): percept is an eval-mode module that offers it.  None otherwise."""
    if not isinstance(percept, nn.Module) or percept.training or not hasattr(percept, method):
        return None
    return getattr(getattr(percept, 'net', None), 'scaling_layer', None)


class PerceptualLoss(nn.Module):
    """`lpips.PerceptualLoss(model='net-lin', net='vgg', ...)` of the reference's Module_Fix_Setup; returns [N,1,1,1]."""

    def __init__(self, model='net-lin', net='vgg', colorspace='rgb', spatial=False, use_gpu=True, gpu_ids=(0,)):
        super().__init__()
        if model != 'net-lin' or net not in ('vgg', 'vgg16') or spatial:
            raise ValueError('only the configuration the training step uses is provided: net-lin / vgg, non-spatial')
        self.net = PNetLin(use_dropout=True)
        self.eval().requires_grad_(False)

    def forward(self, pred, target, normalize=False):
        if normalize:
            target, pred = 2 * target - 1, 2 * pred - 1
        return self.net(target, pred)

    def forward_scaled(self, pred_s, target_s):
        """forward on inputs that are already scaled (ScalingLayer applied): the same argument order."""
        return self.net.forward_scaled(target_s, pred_s)

    def target_features(self, target_s):
        """The trunk taps of a scaled target, detached: computed once for a target that stays (image projection)."""
        with torch.no_grad():
            return [f.detach() for f in self.net.features_scaled(target_s)]

    def forward_cached(self, pred_s, target_feats):
        """forward_scaled(pred_s, target_s) with target_feats = target_features(target_s): the same argument order inside
        (the target's features are f0, the prediction's f1), one trunk pass instead of two."""
        return self.net.forward_features(target_feats, pred_s)
