"""Quantitative-evaluation cases shared by tools/make_golden_quant_eval.py (reference side) and the tests: Generator(256,
512, 8), 256^2 inputs.  Fixture: tests/golden/quant_eval.npz (per-sample values and means, fp32 and float64).

Photos are U(-1,1).  Renders are U(-1,1) inside a centred rectangle and exactly -1 outside it (the background value of
the render mask): 30-60 % of the pixels are outside the mask."""
import synth

QUANT_EVAL_CASES = [
    # the reference's own Get_Recon_Score: two batches of 2 and 1 (photo, render) pairs
    dict(name='recon_256', kind='recon', batches=[2, 1], tsr_encode='Photo Image', sliced_layer=None, use_tanh=False),
    # one batch: `photos` photos, each edited by `renders` renders
    dict(name='edit_256', kind='edit', photos=2, renders=2, tsr_encode='Photo Image', sliced_layer=None, use_tanh=False),
    dict(name='edit_256_render_tanh', kind='edit', photos=1, renders=2, tsr_encode='Render Image',
         sliced_layer=list(range(4, 14)), use_tanh=True),
]
# Compute_Face_Identity_Similarity alone (no generator: runs on the CPU in the tests too): a target and two output batches
IDENTITY_CASE = dict(name='identity_256', b=2)


def identity_inputs(c=IDENTITY_CASE):
    """(target, [output_0, output_1]), each [b,3,256,256] U(-1,1); output_1 is close to the target (similarity near 1)."""
    target = synth.tensor(c['name'] + '/target', (c['b'], 3, 256, 256), dist='uniform')
    out0 = synth.tensor(c['name'] + '/out0', (c['b'], 3, 256, 256), dist='uniform')
    out1 = target + 0.25 * synth.tensor(c['name'] + '/out1', (c['b'], 3, 256, 256), dist='uniform')
    return target, [out0, out1]


# face rectangles (y0, y1, x0, x1) of the renders, cycled: 43.8 %, 48.4 % and 50.6 % of the pixels outside
RECTS = [(32, 224, 32, 224), (32, 224, 40, 216), (40, 216, 40, 224)]


def render(name, n, index=0):
    """[n,3,256,256] renders: U(-1,1) inside RECTS[index % 3], exactly -1 outside."""
    r = synth.tensor(name, (n, 3, 256, 256), dist='uniform')
    y0, y1, x0, x1 = RECTS[index % len(RECTS)]
    out = r.new_full(r.shape, -1.0)
    out[:, :, y0:y1, x0:x1] = r[:, :, y0:y1, x0:x1]
    outside = 1.0 - (y1 - y0) * (x1 - x0) / (256.0 * 256.0)
    assert 0.3 <= outside <= 0.6
    return out


def recon_loader(c):
    """List of (photo, render) batches of the sizes c['batches']."""
    n = sum(c['batches'])
    p = synth.tensor(c['name'] + '/photo', (n, 3, 256, 256), dist='uniform')
    r = render(c['name'] + '/render', n)
    out, i = [], 0
    for b in c['batches']:
        out.append((p[i:i + b].clone(), r[i:i + b].clone()))
        i += b
    return out


def edit_loader(c):
    """One batch [photo, render_1, .., render_n], each [photos,3,256,256]."""
    p = synth.tensor(c['name'] + '/photo', (c['photos'], 3, 256, 256), dist='uniform')
    return [[p] + [render(f"{c['name']}/render{i}", c['photos'], i) for i in range(c['renders'])]]
