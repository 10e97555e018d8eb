"""Re-animation cases shared by tools/make_golden_reanimate.py (reference side) and the tests: ONE photo, `frames` renders,
Generator(256, 512, 8), 256^2 inputs.  Fixture: tests/golden/reanimate.npz (strided sample, stats, float64 sample)."""
import synth

REANIMATE_CASES = [
    dict(name='reanim_256', size=256, frames=3, tsr_encode='Photo Image', sliced_layer=None, use_tanh=False, stride=8),
    dict(name='reanim_256_render_tanh', size=256, frames=2, tsr_encode='Render Image', sliced_layer=list(range(4, 14)),
         use_tanh=True, stride=8),
]


def inputs(c):
    """(photo [1,3,256,256], renders [frames,3,256,256]) of a case, U(-1,1)."""
    p = synth.tensor(c['name'] + '/photo', (1, 3, 256, 256), dist='uniform')
    r = synth.tensor(c['name'] + '/render', (c['frames'], 3, 256, 256), dist='uniform')
    return p, r
