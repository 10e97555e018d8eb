"""Drop-in for the reference's `op` package (op/__init__.py:10-11): same three public names,
backed by hand-written gfx950 kernels in libfmgan_hip.so instead of JIT-compiled CUDA; plus the LPIPS distance of
one VGG tap (lpips/__init__.py), which the reference computes with aten ops."""
from .fused_act import FusedLeakyReLU, fused_leaky_relu
from .lpips_distance import lpips_distance, lpips_distance_serves
from .upfirdn2d import upfirdn2d

__all__ = ['FusedLeakyReLU', 'fused_leaky_relu', 'upfirdn2d', 'lpips_distance', 'lpips_distance_serves']
