#!/usr/bin/env python3
"""Frames/s of re-animating ONE photo with a sequence of renders in the 2-encoder scheme's concatenating modes
('Concatenation', 'Tensor Transform'), three ways, in alternating launches of one process:

  (a) photo_repeated   Forward_Inference(photo repeated over the chunk, renders) — both encoders per frame: the
                       reference's loop structure, the baseline
  (b) reanimate        Encode_Photo_2_Encoder once, Forward_Inference_Reanimate_2_Encoder per chunk, styles per layer
                       from materialised concatenated columns (STYLE_BANK off)
  (c) reanimate_bank   the same with the concatenating style bank (fmgan_style_bank_concat_f32 + fmgan_demod_bank_f32)

    python tools/bench_two_encoder.py [--frames 64] [--rounds 7] [--configs 256:1,1024:8] [--out profiles/two_encoder.md]

Every round runs each leg once over all frames (chunk by chunk, one device synchronise at the end; legs (b) and (c)
include the photo's encoding); the legs alternate inside a round, so drift of the box hits all three alike.  Reported
per leg: median, min and max frames/s over the rounds, and the style + demodulation launches of one Generator forward
(counted on the bindings: equal_linear + modconv_demod per layer, or the two bank launches).  Needs a GPU; prints one JSON
line per configuration and a markdown table, which --out also writes to a file."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: E402

import synth  # noqa: E402
import two_encoder_cases as tc  # noqa: E402
import resnet_encoder  # noqa: E402
import stylegan2  # noqa: E402
from op import _native  # noqa: E402
from psp_encoder_model.encoders import psp_encoders  # noqa: E402
from Util.network_util import (Encode_Photo_2_Encoder, Forward_Inference,  # noqa: E402
                               Forward_Inference_Reanimate_2_Encoder, Reanimate_From_Codes_2_Encoder)

LEGS = ('photo_repeated', 'reanimate', 'reanimate_bank')
MODES = ('Concatenation', 'Tensor Transform')
COUNTED = ('equal_linear', 'modconv_demod', 'style_bank_concat', 'demod_bank')


def run_leg(leg, mode, photo, renders, chunk, e_tsr, e_w, g):
    """All frames once; returns the last chunk's image (kept alive until the caller synchronises)."""
    img = None
    with torch.no_grad():
        if leg == 'photo_repeated':
            for i in range(0, renders.shape[0], chunk):
                r = renders[i:i + chunk]
                img = Forward_Inference(photo.expand(r.shape[0], -1, -1, -1).contiguous(), r, e_tsr, e_w, g,
                                        co_modulation=mode)
            return img
        stylegan2.STYLE_BANK = leg == 'reanimate_bank'
        code = Encode_Photo_2_Encoder(photo, e_tsr, e_w, co_modulation=mode)
        for i in range(0, renders.shape[0], chunk):
            img = Forward_Inference_Reanimate_2_Encoder(code, renders[i:i + chunk], e_tsr, e_w, g, co_modulation=mode)
    return img


@contextlib.contextmanager
def counted():
    """Calls of the style / demodulation bindings inside the block."""
    n = {k: 0 for k in COUNTED}
    orig = {k: getattr(_native, k) for k in n}

    def wrap(k):
        def f(*a, **kw):
            n[k] += 1
            return orig[k](*a, **kw)
        return f
    try:
        for k in n:
            setattr(_native, k, wrap(k))
        yield n
    finally:
        for k in n:
            setattr(_native, k, orig[k])


def generator_launches(leg, mode, photo, renders, chunk, e_tsr, e_w, g):
    """Style + demodulation launches of ONE Generator forward of the leg: both encoders run before the count starts."""
    with torch.no_grad():
        stylegan2.STYLE_BANK = leg == 'reanimate_bank'
        code = Encode_Photo_2_Encoder(photo, e_tsr, e_w, co_modulation=mode)
        frame_code = e_tsr(renders[:chunk])
        with counted() as n:
            Reanimate_From_Codes_2_Encoder(code, frame_code, g, co_modulation=mode)
    return sum(n.values())


def measure(mode, size, chunk, frames, rounds, dev):
    c = dict(size=size, co_mod=mode, mod_space='W+')
    e_tsr, e_w, g = (m.to(dev) for m in tc.build(c, resnet_encoder, psp_encoders, stylegan2))
    photo = synth.tensor('bench_two_encoder/photo', (1, 3, 256, 256), dist='uniform').to(dev)
    renders = synth.tensor('bench_two_encoder/renders', (frames, 3, 256, 256), dist='uniform').to(dev)
    args = (mode, photo, renders, chunk, e_tsr, e_w, g)
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
    res = dict(mode=mode, size=size, chunk=chunk, frames=frames, rounds=rounds, device=torch.cuda.get_device_name(dev))
    for leg in LEGS:
        v = fps[leg]
        res[leg] = dict(median=statistics.median(v), min=min(v), max=max(v))
    res['launches'] = {leg: generator_launches(leg, *args) for leg in LEGS[1:]}
    torch.cuda.synchronize()
    return res


def table(results):
    lines = ['| mode | size | chunk | ' + ' | '.join(f'{leg} frames/s (min .. max)' for leg in LEGS) +
             ' | style + demod launches per forward: per layer / bank |',
             '|---|---|---|' + '---|' * (len(LEGS) + 1)]
    for r in results:
        cells = ' | '.join(f"{r[l]['median']:.1f} ({r[l]['min']:.1f} .. {r[l]['max']:.1f})" for l in LEGS)
        lines.append(f"| {r['mode']} | {r['size']}² | {r['chunk']} | {cells} | "
                     f"{r['launches']['reanimate']} / {r['launches']['reanimate_bank']} |")
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--configs', default='256:1,1024:8', help='size:chunk, comma separated')
    ap.add_argument('--modes', default=','.join(MODES), help='co-modulation modes, comma separated')
    ap.add_argument('--out', default=None, help='also write the table (markdown, with the JSON lines) to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_two_encoder.py measures on a GPU; none is visible')
    dev = torch.device('cuda', 0)
    prev = stylegan2.STYLE_BANK
    results = []
    try:
        for cfg in a.configs.split(','):
            size, chunk = (int(x) for x in cfg.split(':'))
            for mode in a.modes.split(','):
                results.append(measure(mode, size, chunk, a.frames, a.rounds, dev))
                print(json.dumps(results[-1]), flush=True)
    finally:
        stylegan2.STYLE_BANK = prev
    text = table(results)
    print('\n' + text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n\n```\n' + '\n'.join(json.dumps(r) for r in results) + '\n```\n')


if __name__ == '__main__':
    main()
