"""Writes tests/golden/lbfgs.npz: the cases of tests/lbfgs_cases.py run on the reference's FullBatchLBFGS, in float32 and
in float64.  Outputs only.

    python tools/make_golden_lbfgs.py --reference <the reference's Evaluation/image_projection/LBFGS.py>

The reference's file is imported by path (it needs torch and numpy only); nothing of it is copied.  Every case must take
the same line-search decisions in both precisions at every recorded step, or the script stops: a test must never have to
excuse a step because the decisions differ.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import lbfgs_cases as lc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'lbfgs.npz'))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location('reference_lbfgs', args.reference)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.set_num_threads(1)
    out = {}
    for name, case in lc.CASES.items():
        r32, s32, _ = lc.run_case(case, ref.FullBatchLBFGS, torch.float32)
        r64, s64, _ = lc.run_case(case, ref.FullBatchLBFGS, torch.float64)
        for k in lc.DECISIONS:
            assert np.array_equal(r32[k], r64[k]), (name, k, r32[k], r64[k])
        assert r32['curv_skips'] == r64['curv_skips'] and r32['fail_skips'] == r64['fail_skips'], name
        if case.get('wants') == 'curv_skips':
            assert r64['curv_skips'] >= 1, (name, 'no curvature pair was skipped')
        if case.get('wants') == 'fail':
            assert r64['fail'].sum() >= 1, (name, 'no line search failed')
        if case.get('history_size') == 3:
            assert (r64['history'] == 3).sum() >= 5, (name, 'the ring does not wrap')
        if case.get('line_search') == 'Armijo':     # polyinterp's three-point form is the bisection here
            assert r64['ls_step'].max() <= 2, (name, r64['ls_step'])
        for k in ('loss', 't', 'x'):
            out[f'{name}/{k}/f32'] = r32[k]
            out[f'{name}/{k}/f64'] = r64[k]
        for k in lc.DECISIONS:
            out[f'{name}/{k}'] = r64[k]
        out[f'{name}/skips'] = np.array([r64['curv_skips'], r64['fail_skips']])
        dev = np.abs(r32['x'].astype(np.float64) - r64['x']).max()
        print(f"{name}: steps {case['steps']} ls_step {r64['ls_step'].tolist()} history {r64['history'].tolist()} "
              f"skips {out[f'{name}/skips'].tolist()} fail {r64['fail'].tolist()} max|x| {np.abs(r64['x']).max():.3f} "
              f"fp32-fp64 {dev:.2e} loss {r64['loss'][-1]:.4e}")
        for j, st in s32.items():
            d64 = lc.two_loop_f64(st['S'], st['Y'], st['g'], st['H_diag'])
            # the same recursion by the reference's own method, in float64 on the same float32 state
            p = [torch.zeros(st['g'].size, dtype=torch.float64, requires_grad=True)]
            o = ref.LBFGS(p, dtype=torch.float64)
            gs = o.state['global_state']
            gs['old_dirs'] = [torch.from_numpy(v).double() for v in st['S']]
            gs['old_stps'] = [torch.from_numpy(v).double() for v in st['Y']]
            gs['H_diag'] = st['H_diag']
            d_ref = o.two_loop_recursion(-torch.from_numpy(st['g']).double()).numpy()
            assert np.abs(d_ref - d64).max() <= 1e-12 * max(np.abs(d_ref).max(), 1), (name, j)
            for k in ('S', 'Y', 'g', 'd'):
                out[f'{name}/state{j}/{k}'] = st[k]
            out[f'{name}/state{j}/H_diag'] = np.float64(st['H_diag'])
            out[f'{name}/state{j}/d64'] = d_ref
            print(f"  state {j}: k {len(st['S'])} direction fp32-fp64 {np.abs(st['d'] - d_ref).max():.2e} of "
                  f"{np.abs(d_ref).max():.2e}")
    for i, (points, lo, hi) in enumerate(lc.POLYINTERP):
        out[f'polyinterp/{i}'] = np.float64(ref.polyinterp(np.array(points), lo, hi))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
