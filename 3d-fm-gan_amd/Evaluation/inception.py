"""Inception v3 in the FID variant (reference Evaluation/inception.py: pytorch-fid's wrapper round torchvision's
Inception3 with the patched FID blocks), written out from the architecture: torchvision is not a dependency.

    InceptionV3(output_blocks=[3], resize_input=True, normalize_input=True, requires_grad=False, weights=None)
    forward(inp) -> list of the selected blocks' outputs, ascending:
        0   input .. first max pool            [B,   64, 73, 73]
        1   .. second max pool                 [B,  192, 35, 35]
        2   Mixed_5b .. Mixed_6e (pre-aux)     [B,  768, 17, 17]
        3   Mixed_7a .. global average pool    [B, 2048,  1,  1]
    Sizes 299 -> 149 -> 147 -> 73 -> 71 -> 35 -> 17 -> 8; channels 192 / 256 / 288 (Mixed_5*) / 768 (Mixed_6*) / 1280 /
    2048 (Mixed_7*).

FID patches (the TensorFlow graph the published weights come from): the 3x3 average pools of the A, C and first E blocks
use count_include_pad=False, the last E block pools with a max, and `fc` is 1008-way (never evaluated here, kept so that
the checkpoint loads).

Weights: parameter and buffer names are torchvision's Inception3 names (Conv2d_1a_3x3.conv.weight,
Mixed_5b.branch1x1.bn.running_var, ..., fc.weight), so a torch.load of the published pt_inception FID checkpoint goes in
through `weights=` (or load_weights / load_state_dict).  Neither torchvision nor the checkpoint is available where this
is developed, so the key list is written from the architecture and is NOT pinned by a fixture: `load_weights` is strict
about everything except BatchNorm's num_batches_tracked (filled in when absent) and an AuxLogits.* head (dropped when
present).  weights=None keeps the module's own initialisation: features of such a network are a load figure, not an FID.

Inference path: under torch.no_grad() in eval mode the forward runs BatchNorm folded into each convolution (once per
weight version), in channels_last throughout, behind the fused input stage (op/inception_input.py) where that serves;
everything else (training mode, autograd) takes the module-by-module form after the composite input stage.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from op.inception_input import inception_input


class BasicConv2d(nn.Module):
    """Convolution without bias + BatchNorm2d(eps=0.001) + ReLU."""

    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)
        self._folded = None

    def _key(self):
        ts = (self.conv.weight, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var)
        return tuple((t.data_ptr(), t._version, t.dtype, t.device) for t in ts)

    def folded(self):
        """(weight, bias) of the convolution with the eval-mode BatchNorm folded in, computed once per weight version."""
        key = self._key()
        if self._folded is None or self._folded[0] != key:
            with torch.no_grad():
                k = self.bn.weight / torch.sqrt(self.bn.running_var + self.bn.eps)
                w = (self.conv.weight * k[:, None, None, None]).contiguous(memory_format=torch.channels_last)
                b = self.bn.bias - self.bn.running_mean * k
            self._folded = (key, w, b)
        return self._folded[1:]

    def forward(self, x, fold=False):
        if fold:
            w, b = self.folded()
            return F.relu_(F.conv2d(x, w, b, self.conv.stride, self.conv.padding))
        return F.relu(self.bn(self.conv(x)), inplace=True)


def _avg3(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


class InceptionA(nn.Module):
    def __init__(self, in_channels, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(in_channels, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(in_channels, pool_features, kernel_size=1)

    def forward(self, x, fold=False):
        b1 = self.branch1x1(x, fold)
        b5 = self.branch5x5_2(self.branch5x5_1(x, fold), fold)
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x, fold), fold), fold)
        bp = self.branch_pool(_avg3(x), fold)
        return torch.cat([b1, b5, b3, bp], 1)


class InceptionB(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_channels, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x, fold=False):
        b3 = self.branch3x3(x, fold)
        bd = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x, fold), fold), fold)
        return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, in_channels, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)

    def forward(self, x, fold=False):
        b1 = self.branch1x1(x, fold)
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x, fold), fold), fold)
        bd = self.branch7x7dbl_1(x, fold)
        for m in (self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5):
            bd = m(bd, fold)
        bp = self.branch_pool(_avg3(x), fold)
        return torch.cat([b1, b7, bd, bp], 1)


class InceptionD(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x, fold=False):
        b3 = self.branch3x3_2(self.branch3x3_1(x, fold), fold)
        b7 = self.branch7x7x3_1(x, fold)
        for m in (self.branch7x7x3_2, self.branch7x7x3_3, self.branch7x7x3_4):
            b7 = m(b7, fold)
        return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    """pool='avg': the first E block (average without the padding); pool='max': the last one, as the FID graph has it."""

    def __init__(self, in_channels, pool='avg'):
        super().__init__()
        self.pool = pool
        self.branch1x1 = BasicConv2d(in_channels, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(in_channels, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)

    def forward(self, x, fold=False):
        b1 = self.branch1x1(x, fold)
        b3 = self.branch3x3_1(x, fold)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x, fold), fold)
        pooled = _avg3(x) if self.pool == 'avg' else F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
        bp = self.branch_pool(pooled, fold)
        return torch.cat([b1, self.branch3x3_2a(b3, fold), self.branch3x3_2b(b3, fold),
                          self.branch3x3dbl_3a(bd, fold), self.branch3x3dbl_3b(bd, fold), bp], 1)


# the layers of each output block, by attribute name; None: the 3x3 stride-2 max pool that ends blocks 0 and 1
BLOCKS = (
    ('Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3', None),
    ('Conv2d_3b_1x1', 'Conv2d_4a_3x3', None),
    ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'),
    ('Mixed_7a', 'Mixed_7b', 'Mixed_7c'),
)


class InceptionV3(nn.Module):
    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True,
                 requires_grad=False, weights=None):
        super().__init__()
        self.resize_input = resize_input
        self.normalize_input = normalize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        if min(output_blocks) < 0 or self.last_needed_block > 3:
            raise ValueError('output_blocks: the last possible output block index is 3')
        self._fold_allowed = True
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, channels_7x7=128)
        self.Mixed_6c = InceptionC(768, channels_7x7=160)
        self.Mixed_6d = InceptionC(768, channels_7x7=160)
        self.Mixed_6e = InceptionC(768, channels_7x7=192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, pool='avg')
        self.Mixed_7c = InceptionE(2048, pool='max')
        self.fc = nn.Linear(2048, 1008)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, nonlinearity='relu')
        if weights is not None:
            self.load_weights(weights)
        for param in self.parameters():
            param.requires_grad = requires_grad

    def load_weights(self, state_dict):
        """load_state_dict of a checkpoint in torchvision's Inception3 naming (the published FID weights): strict, except
        that missing num_batches_tracked buffers are filled in and an AuxLogits.* head is dropped."""
        own = self.state_dict()
        sd = {k: v for k, v in state_dict.items() if not k.startswith('AuxLogits.')}
        for k, v in own.items():
            if k.endswith('num_batches_tracked') and k not in sd:
                sd[k] = v
        return self.load_state_dict(sd, strict=True)

    def _folds(self, inp):
        return self._fold_allowed and not torch.is_grad_enabled() and not self.training

    def forward(self, inp, fuse=True):
        """The list of the selected blocks' outputs.  fuse=False keeps the composite input stage."""
        fold = self._folds(inp)
        if fold:
            x = inception_input(inp, self.normalize_input, self.resize_input, fuse=fuse)
        else:
            x = inp
            if self.resize_input:
                x = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False)
            if self.normalize_input:
                x = 2 * x - 1
        outp = []
        for idx, names in enumerate(BLOCKS):
            for name in names:
                x = F.max_pool2d(x, kernel_size=3, stride=2) if name is None else getattr(self, name)(x, fold)
            if idx == 3:
                x = F.adaptive_avg_pool2d(x, (1, 1))
            if idx in self.output_blocks:
                outp.append(x)
            if idx == self.last_needed_block:
                break
        return outp

    def forward_modules(self, inp):
        """The module-by-module form (no folding, no fused input stage), whatever the mode: the baseline of the tests and
        of tools/bench_fid.py."""
        self._fold_allowed = False
        try:
            return self.forward(inp)
        finally:
            self._fold_allowed = True
