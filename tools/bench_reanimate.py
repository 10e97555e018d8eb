#!/usr/bin/env python3
"""Frames/s of re-animating ONE photo with a sequence of renders, three ways, in alternating launches of one process:

  (a) photo_repeated   Forward_Inference_3_Encoder(photo repeated over the chunk, renders)  — all three encoders per frame
  (b) reanimate        Encode_Photo once, Forward_Inference_Reanimate per chunk, styles per layer (FMGAN_NO_STYLE_BANK=1)
  (c) reanimate_bank   the same with the two-launch style bank

    python tools/bench_reanimate.py [--frames 64] [--rounds 7] [--configs 256:1,256:32,1024:8] [--out profiles/x.json]

Every round runs each leg once over all frames (chunk by chunk, one device synchronise at the end; legs (b) and (c)
include the photo's encoding); the legs alternate inside a round, so drift of the box hits all three alike.  Reported
per leg: median, min and max frames/s over the rounds.  Needs a GPU; prints one JSON line per configuration and a
markdown table."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: E402

import synth  # noqa: E402
import resnet_encoder  # noqa: E402
import stylegan2  # noqa: E402
from psp_encoder_model.encoders import psp_encoders  # noqa: E402
from Util.network_util import Encode_Photo, Forward_Inference_3_Encoder, Forward_Inference_Reanimate  # noqa: E402

LEGS = ('photo_repeated', 'reanimate', 'reanimate_bank')


def build(size, dev):
    n_latent = 2 * (size.bit_length() - 1) - 2
    nets = [('resnet', resnet_encoder.resnet18(tensor_encoding=True, tensor_transform=False), 5),
            ('resnet', resnet_encoder.resnet18(tensor_encoding=False, tensor_transform=False), 6),
            ('psp', psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=n_latent)), 7),
            ('generator', stylegan2.Generator(size, 512, 8), 4)]
    out = []
    for kind, m, seed in nets:
        m.load_state_dict(synth.state_dict(kind, m.state_dict(), seed=seed))
        out.append(m.to(dev).eval())
    return out


def run_leg(leg, photo, renders, chunk, e_tsr, e_w, e_wp, g):
    """All frames once; returns the last chunk's image (kept alive until the caller synchronises)."""
    img = None
    with torch.no_grad():
        if leg == 'photo_repeated':
            for i in range(0, renders.shape[0], chunk):
                r = renders[i:i + chunk]
                img = Forward_Inference_3_Encoder(photo.expand(r.shape[0], -1, -1, -1).contiguous(), r, e_tsr, e_w, e_wp, g)
            return img
        stylegan2.STYLE_BANK = leg == 'reanimate_bank'
        code = Encode_Photo(photo, e_tsr, e_wp)
        for i in range(0, renders.shape[0], chunk):
            img = Forward_Inference_Reanimate(code, renders[i:i + chunk], e_tsr, e_w, g)
    return img


def measure(size, chunk, frames, rounds, dev):
    e_tsr, e_w, e_wp, g = build(size, dev)
    photo = synth.tensor('bench_reanimate/photo', (1, 3, 256, 256), dist='uniform').to(dev)
    renders = synth.tensor('bench_reanimate/renders', (frames, 3, 256, 256), dist='uniform').to(dev)
    args = (photo, renders, chunk, e_tsr, e_w, e_wp, g)
    for _ in range(2):                      # every shape of the timed window: library algorithm search, placement selection
        for leg in LEGS:
            run_leg(leg, *args)
    torch.cuda.synchronize()
    fps = {leg: [] for leg in LEGS}
    for rnd in range(rounds):
        order = LEGS if rnd % 2 == 0 else LEGS[::-1]
        for leg in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_leg(leg, *args)
            torch.cuda.synchronize()
            fps[leg].append(frames / (time.perf_counter() - t0))
    res = dict(size=size, chunk=chunk, frames=frames, rounds=rounds, device=torch.cuda.get_device_name(dev))
    for leg in LEGS:
        v = fps[leg]
        res[leg] = dict(median=statistics.median(v), min=min(v), max=max(v))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--configs', default='256:1,256:32,1024:8', help='size:chunk, comma separated')
    ap.add_argument('--out', default=None, help='also write the results as JSON to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_reanimate.py measures on a GPU; none is visible')
    dev = torch.device('cuda', 0)
    prev = stylegan2.STYLE_BANK
    results = []
    try:
        for cfg in a.configs.split(','):
            size, chunk = (int(x) for x in cfg.split(':'))
            results.append(measure(size, chunk, a.frames, a.rounds, dev))
            print(json.dumps(results[-1]), flush=True)
    finally:
        stylegan2.STYLE_BANK = prev
    print('\n| size | chunk | ' + ' | '.join(f'{leg} frames/s (min .. max)' for leg in LEGS) + ' |')
    print('|---|---|' + '---|' * len(LEGS))
    for r in results:
        cells = ' | '.join(f"{r[l]['median']:.1f} ({r[l]['min']:.1f} .. {r[l]['max']:.1f})" for l in LEGS)
        print(f"| {r['size']}² | {r['chunk']} | {cells} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(results, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
