"""Seeded operands of the bf16 / split-operand modulated-conv tests (not a conftest: a plain helper, imported by name),
shared by tests/test_hip_modconv_bf16.py and tests/test_hip_modconv_bf16_edges.py."""
import numpy as np

import synth


def inputs(cfg):
    """cfg = (b, cin, cout, h, w, mode) -> (x, weight, style, scale) on the CPU: N(0,1) activations and weights, styles
    around 1, the equalised-lr scale 1/sqrt(cin*9) as the fp32 number the layers pass."""
    b, cin, cout, h, w, mode = cfg
    x = synth.tensor(f'bf/{cfg}/x', (b, cin, h, w))
    wgt = synth.tensor(f'bf/{cfg}/w', (cout, cin, 3, 3))
    s = synth.tensor(f'bf/{cfg}/s', (b, cin), shift=1.0, scale=0.5)
    return x, wgt, s, float(np.float32(1.0 / np.sqrt(cin * 9)))
