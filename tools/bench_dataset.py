#!/usr/bin/env python3
"""The data side on the GPU (op/image_bank.py, dataset.BankLoader) against the parent's means and the reference's structure.

    python tools/bench_dataset.py [--rounds R] [--window S] [--json PATH] [--md PATH]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_dataset.py --kernel-only      (measurement 2)

1. The training triple (g_input, r_input, g_ref) at [16, 3, 256, 256] and [32, 3, 256, 256], for a reconstruction, a
   dual-supervision and an extreme-pose batch (the last from twice as many positions, as train() asks): `fused` is
   BankLoader.training_batch, one launch; `composite` is what the parent commit offers on the same device-resident
   bytes: index_select of the uint8 banks, Util.image_io.images_to_tensor, then Data_Loading's clone / pair swap / even
   members on the float tensors.  `fused P=4` / `fused P=16` are the raw entry with the lane's pixel run forced.
2. The kernel alone (--kernel-only, under rocprofv3): the triple of a 16-batch (n = 48 images, cache-resident: input
   and output fit the 256 MiB Infinity Cache and the windows re-read them) and n = 512 images of 256^2 out of a bank of
   1024 (input + output 503 MB), at P = 4 and P = 16.  Algorithmic bytes are n * H * W * 15.  The same launches are also
   timed here with HIP events (`kernel` rows), back to back, so their figure includes the launch gaps.
3. Images per second of the reference's structure, DataLoader(num_workers=8) over PNG files with Transform, against the
   bank loader over the same files; the bank's fill time (decode + upload) is reported separately.  Without PIL this
   leg is reported as not measured.
Method: HIP events round a window of back-to-back calls lasting at least --window seconds; every version warmed up; the
versions alternate inside each of R rounds; per call: the median round, the lowest and the highest (tools/bench_ppl.py).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-fm-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dataset  # noqa: E402
from bench_ppl import alternate  # noqa: E402
from op import _native, image_bank  # noqa: E402
from op.image_bank import EpochIndex, ImageBank  # noqa: E402
from Util import image_io  # noqa: E402

HBM_PEAK_GBS = 8000.0
SIZE = 256
TRIPLE = {'reconstruction': [(0, 0, 0, 1, 0), (1, 0, 0, 1, 0), (0, 0, 0, 1, 0)],      # raw: (bank, source, swap, mul, add)
          'dual supervision': [(0, 0, 0, 1, 0), (1, 0, 1, 1, 0), (0, 0, 1, 1, 0)]}


def random_bank(n, device, seed):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(device)


def composite_triple(banks, order, offset, batch, mode):
    idx = order[offset:offset + batch].long()
    stream = iter([(image_io.images_to_tensor(banks[0].index_select(0, idx)),
                    image_io.images_to_tensor(banks[1].index_select(0, idx)))])
    ds, ep = mode != 'reconstruction', mode == 'extreme pose'
    return dataset.Data_Loading(stream, stream, ds, banks[0].device, extreme_loader=stream, extreme_ds_flag=ep)


def triple_rows(d, rounds, window):
    banks = [random_bank(1024, d, 1), random_bank(1024, d, 2)]
    res = dataset.Resident.from_banks('pair', banks)
    order = torch.randperm(1024, generator=torch.Generator().manual_seed(3))
    index = EpochIndex(order.tolist() * 2, 1024, d)
    rows = []
    for batch in (16, 32):
        for mode in ('reconstruction', 'dual supervision', 'extreme pose'):
            positions = 2 * batch if mode == 'extreme pose' else batch
            groups = TRIPLE['reconstruction' if mode == 'reconstruction' else 'dual supervision']
            stride = 2 if mode == 'extreme pose' else 1
            loader = dataset.BankLoader(res, positions, torch.utils.data.SequentialSampler(res))
            loader._index, loader._order = index, list(range(len(index)))

            def fused():
                loader._cursor = 64
                return loader.training_batch(pair=mode != 'reconstruction', even_only=mode == 'extreme pose')

            def forced(pix):
                return lambda: _native.bank_gather(banks, index.data, None, 64, positions // stride, stride, groups,
                                                   pixels_per_lane=pix)
            a, b = fused(), composite_triple(banks, index.data, 64, positions, mode)
            assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape[0] == batch
            got = alternate({'fused': fused, 'composite': lambda: composite_triple(banks, index.data, 64, positions, mode),
                             'fused P=4': forced(4), 'fused P=16': forced(16)}, rounds, window)
            for name, (med, lo, hi, calls) in got.items():
                rows.append(dict(measurement='triple', shape=f'[{batch}, 3, 256, 256]', mode=mode, version=name, us=med,
                                 lowest=lo, highest=hi, calls=calls))
                print(rows[-1], flush=True)
    return rows


def kernel_cases(d):
    """(label, n, launch(pix)) of measurement 2; outputs preallocated, the launch through the raw wrapper."""
    banks = [random_bank(1024, d, 1), random_bank(1024, d, 2)]
    order = torch.randperm(1024, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(d)
    cases = []
    for label, members, groups in (('n = 48 (16-batch triple, cache-resident)', 16, TRIPLE['dual supervision']),
                                   ('n = 512', 256, [(0, 0, 0, 1, 0), (1, 0, 0, 1, 0)])):
        n = members * len(groups)
        out = torch.empty((n, 3, SIZE, SIZE), device=d)

        def launch(pix, members=members, groups=groups, out=out):
            _native.bank_gather(banks, order, None, 0, members, 1, groups, out=out, pixels_per_lane=pix)
        cases.append((label, n, launch))
    return cases


def kernel_rows(d, rounds, window):
    rows = []
    for label, n, launch in kernel_cases(d):
        got = alternate({f'kernel P={pix}': (lambda pix=pix: launch(pix)) for pix in (4, 16)}, rounds, window)
        for name, (med, lo, hi, calls) in got.items():
            gbs = n * SIZE * SIZE * 15 / med / 1e3
            rows.append(dict(measurement='kernel (HIP events, back to back)', shape=label, version=name, us=med, lowest=lo,
                             highest=hi, calls=calls, gbs=round(gbs, 1), of_peak=round(gbs / HBM_PEAK_GBS, 4)))
            print(rows[-1], flush=True)
    return rows


def kernel_only(d, reps=20):
    """For a rocprofv3 --kernel-trace --stats run: each case `reps` times at each P, synchronised between the cases so
    that the trace groups by kernel name (bank_gather_vec_k<4> / <16>) and case order."""
    for label, n, launch in kernel_cases(d):
        for pix in (4, 16):
            for _ in range(reps):
                launch(pix)
            torch.cuda.synchronize()
            print(f'{label}: P = {pix}, n = {n}, {reps} launches, {n * SIZE * SIZE * 15} algorithmic bytes each', flush=True)


def loader_rows(d, n_items=256, batch=16):
    try:
        from PIL import Image
    except ImportError:
        return [dict(measurement='loader', version='DataLoader(num_workers=8) and bank loader', note='not measured: PIL '
                     'is not installed on this machine')]
    rows = []
    with tempfile.TemporaryDirectory() as root:
        rng = np.random.RandomState(7)
        yy, xx = np.mgrid[0:SIZE, 0:SIZE]
        for i in range(n_items // 7 + 1):
            os.makedirs(os.path.join(root, f'id_{i}'))
        for i in range(n_items):
            for kind in 'gr':
                # smooth colour fields with a little noise: PNGs of a few tens of kilobytes, as renders are
                base = np.stack([(np.sin(xx / rng.uniform(8, 40) + rng.uniform(0, 6)) +
                                  np.cos(yy / rng.uniform(8, 40))) * 60 + 128 for _ in range(3)], axis=-1)
                a = np.clip(base + rng.randint(-6, 7, base.shape), 0, 255).astype(np.uint8)
                Image.fromarray(a).save(os.path.join(root, f'id_{i // 7}', f'{kind}_{i % 7}.png'))
        ds = dataset.Synthetic_Dataset(root, dataset.Transform(SIZE))
        # fresh worker processes that never touch the GPU, kept across epochs; the first epoch (their start-up) is dropped
        ref = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, num_workers=8,
                                          multiprocessing_context='spawn', persistent_workers=True)
        for g, r in ref:
            pass
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            for g, r in ref:
                g, r = g.to(d), r.to(d)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        del ref                                         # ends the workers
        rows.append(dict(measurement='loader', version='DataLoader(num_workers=8), PIL decode + Transform, float32 to device',
                         images_per_s=round(2 * len(ds) / sorted(times)[1], 1), epochs_s=[round(t, 3) for t in times]))
        print(rows[-1], flush=True)
        t0 = time.perf_counter()
        res = dataset.Resident(ds, SIZE, d)
        torch.cuda.synchronize()
        fill = time.perf_counter() - t0
        rows.append(dict(measurement='loader', version='bank fill (decode once, 8 threads, upload)', seconds=round(fill, 3),
                         images_per_s=round(2 * len(ds) / fill, 1)))
        print(rows[-1], flush=True)
        loader = dataset.BankLoader(res, batch, torch.utils.data.RandomSampler(res))
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(20):
                for g, r in loader:
                    pass
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / 20)
        rows.append(dict(measurement='loader', version='BankLoader (epoch upload + one launch per batch)',
                         images_per_s=round(2 * len(ds) / sorted(times)[1], 1), epochs_s=[round(t, 5) for t in times]))
        print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--json')
    ap.add_argument('--md')
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--skip-loader', action='store_true')
    a = ap.parse_args()
    d = torch.device('cuda', 0)
    if a.kernel_only:
        return kernel_only(d)
    rows = triple_rows(d, a.rounds, a.window) + kernel_rows(d, a.rounds, a.window)
    if not a.skip_loader:
        try:
            rows += loader_rows(d)
        except Exception as e:      # the first two measurements are kept; this leg says why it has no figure
            rows.append(dict(measurement='loader', note=f'not measured: {type(e).__name__}: {e}'))
            print(rows[-1], flush=True)
    out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, window_s=a.window, bank_fuse=image_bank.BANK_FUSE,
               rows=rows)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)
    if a.md:
        keys = ['measurement', 'shape', 'mode', 'version', 'us', 'lowest', 'highest', 'gbs', 'of_peak', 'images_per_s',
                'seconds', 'note']
        with open(a.md, 'w') as f:
            f.write('| ' + ' | '.join(keys) + ' |\n|' + '---|' * len(keys) + '\n')
            for r in rows:
                f.write('| ' + ' | '.join(str(r.get(k, '')) for k in keys) + ' |\n')


if __name__ == '__main__':
    main()
