#!/usr/bin/env python3
"""Two comparisons for the visual-evaluation drivers, each new path against the same work built from the functions that
existed before it, in alternating launches of one process:

  (a) sheet   the composition of Batch_Eval_Sheet for `--sets` sets (photos, renders 256^2; outputs S^2; tile 256):
                new       canvas fill + one tiles_to_canvas per source tensor (3 launches)
                baseline  canvas fill + per tensor F.interpolate (S != 256) + tensor2im_batch, then one slice copy per tile
              the networks are not run: the float images are random.  Reported: microseconds per sheet.
  (b) video   `--frames` photo / render pairs reconstructed at Generator(S), full-width networks:
                new       Reconstruct_Frames(chunk 8): chunked forwards, one conversion and one host copy per chunk
                baseline  the reference's structure: Forward_Inference_3_Encoder at B = 1 + tensor2im per frame
              Reported: frames per second.

    python tools/bench_visual_eval.py [--sizes 256,1024] [--sets 6] [--frames 64] [--rounds 3] [--out profiles/x.json]

Every round runs each leg once (a: `--reps` sheets per leg and round, one device synchronise at the end; b: all frames,
the host copies included); the legs alternate inside a round, the order flips between rounds.  Reported per leg: median,
min and max over the rounds.  Needs a GPU; prints one JSON line per measurement and a markdown table."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import synth  # noqa: E402
from bench_reanimate import build  # noqa: E402
from Evaluation.visual_eval import Reconstruct_Frames, tensor2im, tensor2im_batch  # noqa: E402
from op.canvas import sheet_layout, tiles_to_canvas  # noqa: E402
from Util.network_util import Forward_Inference_3_Encoder  # noqa: E402

TILE, GAP, MARGIN = 256, 8, 8


def alternate(legs, rounds, run):
    """{leg: [seconds per round]}: each leg once per round between device synchronisations, order flipped every round."""
    out = {leg: [] for leg in legs}
    for rnd in range(rounds):
        for leg in (legs if rnd % 2 == 0 else legs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(leg)
            torch.cuda.synchronize()
            out[leg].append(time.perf_counter() - t0)
    return out


def summary(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


# ----------------------------------------------------------------------------------------------------------- (a)
def sheet_new(tensors, slots, shape):
    canvas = torch.full(shape, 255, dtype=torch.uint8, device=tensors[0].device)
    for t, s in zip(tensors, slots):
        tiles_to_canvas(t, canvas, s, TILE)
    return canvas


def sheet_baseline(tensors, slots, shape):
    canvas = torch.full(shape, 255, dtype=torch.uint8, device=tensors[0].device)
    for t, s in zip(tensors, slots):
        if t.shape[-1] != TILE:
            t = F.interpolate(t, size=TILE, mode='bilinear', align_corners=False)
        u8 = tensor2im_batch(t)
        for k, (y0, x0) in enumerate(s):
            canvas[y0:y0 + TILE, x0:x0 + TILE] = u8[k]
    return canvas


def kernel_time(t, slots, shape, reps):
    """(microseconds per launch by device events, bytes read + written) of the raw launch that puts `t` on the sheet:
    slots uploaded once, `reps` launches back to back on one stream."""
    import numpy as np
    from op import _native
    canvas = torch.full((1,) + tuple(shape), 255, dtype=torch.uint8, device=t.device)
    dev_slots = torch.from_numpy(np.asarray([(0, y, x) for y, x in slots], dtype=np.int32)).to(t.device)
    for _ in range(5):
        _native.tiles_to_canvas(t, canvas, dev_slots, TILE)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        _native.tiles_to_canvas(t, canvas, dev_slots, TILE)
    b.record()
    torch.cuda.synchronize()
    f = t.shape[-1] // TILE
    touched = t.numel() * 4 // (1 if f < 4 else 2)          # f = 4 reads the two tap rows of every four
    return 1e3 * a.elapsed_time(b) / reps, touched + t.shape[0] * 3 * TILE * TILE


def measure_sheet(size, sets, rounds, reps, dev):
    h, w, yx = sheet_layout(sets, 5, TILE, GAP, MARGIN)
    yx = yx.reshape(sets, 5, 2)
    slots = [yx[:, 0].tolist(), yx[:, 1::2].reshape(-1, 2).tolist(), yx[:, 2::2].reshape(-1, 2).tolist()]
    tensors = [synth.tensor(f'bench_ve/{n}', (k * sets, 3, s, s), dist='uniform', scale=1.2).to(dev)
               for n, k, s in (('photo', 1, 256), ('render', 2, 256), ('out', 2, size))]
    legs = {'new': sheet_new, 'baseline': sheet_baseline}
    a, b = (legs[l](tensors, slots, (h, w, 3)) for l in ('new', 'baseline'))
    diff = (a.int() - b.int()).abs()
    secs = alternate(('new', 'baseline'), rounds, lambda leg: [legs[leg](tensors, slots, (h, w, 3)) for _ in range(reps)])
    res = dict(what='sheet', size=size, sets=sets, rounds=rounds, reps=reps, device=torch.cuda.get_device_name(dev),
               sheet=[h, w], max_byte_difference=int(diff.max()), bytes_differing=int((diff > 0).sum()))
    for leg in legs:
        res[leg] = summary([1e6 * s / reps for s in secs[leg]])         # microseconds per sheet
    us, nbytes = kernel_time(tensors[2], slots[2], (h, w, 3), reps)     # the outputs' launch alone, on the device
    res['kernel_outputs'] = dict(us=us, bytes=nbytes, gb_per_s=nbytes / us / 1e3)
    return res


# ----------------------------------------------------------------------------------------------------------- (b)
def video_new(p, r, mods):
    return Reconstruct_Frames(p, r, mods, chunk=8)


def video_baseline(p, r, mods):
    e_tsr, e_w, e_wp, g = mods
    out = []
    with torch.no_grad():
        for t in range(p.shape[0]):
            out.append(tensor2im(Forward_Inference_3_Encoder(p[t:t + 1], r[t:t + 1], e_tsr, e_w, e_wp, g)))
    return out


def measure_video(size, frames, rounds, dev):
    mods = tuple(build(size, dev))
    p = synth.tensor('bench_ve/p', (frames, 3, 256, 256), dist='uniform').to(dev)
    r = synth.tensor('bench_ve/r', (frames, 3, 256, 256), dist='uniform').to(dev)
    legs = {'new': video_new, 'baseline': video_baseline}
    for _ in range(2):                      # every shape of the timed window: library algorithm search, placement selection
        for leg in legs:
            n = len(legs[leg](p[:16], r[:16], mods))
            assert n == 16
    secs = alternate(('new', 'baseline'), rounds, lambda leg: legs[leg](p, r, mods))
    res = dict(what='video', size=size, frames=frames, chunk=8, rounds=rounds, device=torch.cuda.get_device_name(dev))
    for leg in legs:
        res[leg] = summary([frames / s for s in secs[leg]])             # frames per second
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='256,1024')
    ap.add_argument('--sets', type=int, default=6)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=200, help='sheets per leg and round in (a)')
    ap.add_argument('--only', choices=('sheet', 'video'), default=None)
    ap.add_argument('--out', default=None, help='also write the results as JSON to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_visual_eval.py measures on a GPU; none is visible')
    dev = torch.device('cuda', 0)
    results = []
    for size in (int(s) for s in a.sizes.split(',')):
        if a.only != 'video':
            measure_sheet(size, a.sets, 1, 5, dev)                      # warm-up of every shape
            results.append(measure_sheet(size, a.sets, a.rounds, a.reps, dev))
            print(json.dumps(results[-1]), flush=True)
        if a.only != 'sheet':
            results.append(measure_video(size, a.frames, a.rounds, dev))
            print(json.dumps(results[-1]), flush=True)
    print('\n| comparison | size | unit | new (min .. max) | baseline (min .. max) |')
    print('|---|---|---|---|---|')
    for r in results:
        unit = 'µs per sheet' if r['what'] == 'sheet' else 'frames/s'
        cells = ' | '.join(f"{r[l]['median']:.1f} ({r[l]['min']:.1f} .. {r[l]['max']:.1f})" for l in ('new', 'baseline'))
        print(f"| {r['what']} | {r['size']}² | {unit} | {cells} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(results, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
