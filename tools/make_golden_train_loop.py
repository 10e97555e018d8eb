"""Writes tests/golden/train_loop.json from the reference's train_3_encoder.py, train_3_encoder_hyperparams.py and
Util/analysis_util.py: names, settings and recorded output only.

    FMGAN_REFERENCE=<the reference's root> python tools/make_golden_train_loop.py

  arguments   every --name of the reference's Args_Parsing with the value of the hyper-parameter it defaults to, read with
              `ast` from the two files (names such as MODULATION_ENCODING[0] are resolved from the literal lists of the
              files they are imported from; np.inf is float('inf'))
  status      for the fixed settings below, the text of Print_Experiment_Status
  lines       for fixed loss values, Print_Train_Status's line for the three flag combinations
  log         a small log made of the status text, those lines, a line in the 2-encoder script's older format (no G_Reg
              field) and two pairs of evaluation blocks — with what the reference's Parse_A_Line (per line; the name of the
              exception where it raises), Moving_Average and the two Extract_* functions return on it

The reference's train_3_encoder.py does not import (its tail is duplicated: a SyntaxError) and analysis_util.py's imports
are not installed here, so only the named functions' source is executed, cut from the text, in a namespace of its own;
reduce_loss_dict is the identity there.  Nothing of the reference's text is copied into the fixture.
"""
import argparse
import ast
import contextlib
import io
import json
import os
import re
import tempfile
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATUS_SETTINGS = dict(synface_dir='data/synface', extreme_pose_dir='data/extreme_pose', ffhq_train_img_dir='data/ffhq/train',
                       quant_eval_img_dir='data/ffhq/val', visual_real_img_dir='data/visual', ckpt=None, device='cuda:0',
                       gpu_device_ids=None, n_latent=14, distributed=False, n_gpu=1)
LOSSES = {'d': 1.23456789, 'r1': 0.0421, 'g_reg': 0.00051234, 'g': 0.6931472, 'lpips': 1.40251, 'l1': 0.3335,
          'face_id': 12.0005, 'hmap': 0.0, 'face_reg': 2.71828}
FLAGS = ((False, False), (True, False), (True, True))
SECONDS = (0.456789, 1.005, 12.3449)
EVAL = ((0.5, 0.25, 0.125, 0.75, 12.5, 0.031, 3.5, 0.0625), (0.625, 0.2, 0.1, 0.8, 9.75, 0.03, 3.25, 0.05))


def cut_function(text, name):
    """The source of top-level function `name`: from its def line to the next top-level statement."""
    m = re.search(r'^def ' + name + r'\(.*?(?=^\S)', text, re.S | re.M)
    assert m, name
    return m.group(0)


def literal_assignments(path):
    out = {}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            try:
                out[node.targets[0].id] = ast.literal_eval(node.value)
            except ValueError:
                pass
    return out


def hyperparams(ref):
    """name -> value of train_3_encoder_hyperparams.py, without importing it."""
    path = os.path.join(ref, 'train_3_encoder_hyperparams.py')
    tree = ast.parse(open(path).read())
    known = {}
    for node in tree.body:
        if isinstance(node, ast.ImportFrom):
            found = literal_assignments(os.path.join(ref, *node.module.split('.')) + '.py')
            for alias in node.names:
                known[alias.asname or alias.name] = found[alias.name]

    def value(node):
        if isinstance(node, ast.Subscript):
            return value(node.value)[value(node.slice)]
        if isinstance(node, ast.Name):
            return known[node.id]
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and (node.value.id, node.attr) == ('np', 'inf'):
            return float('inf')
        return ast.literal_eval(node)

    for node in tree.body:
        if isinstance(node, ast.Assign):
            known[node.targets[0].id] = value(node.value)
    return known


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('FMGAN_REFERENCE'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'train_loop.json'))
    a = ap.parse_args()
    assert a.reference, 'set FMGAN_REFERENCE or pass --reference'
    train_text = open(os.path.join(a.reference, 'train_3_encoder.py')).read()
    hp = hyperparams(a.reference)
    parsing = cut_function(train_text, 'Args_Parsing')
    arguments = {name: hp[var] for name, var in
                 re.findall(r"add_argument\('--(\w+)',[^\n]*?default\s*=\s*train_hyperparams\.(\w+)\)", parsing)}
    assert len(arguments) == len(re.findall(r'add_argument\(', parsing)), len(arguments)

    ns = {'reduce_loss_dict': lambda d: d}
    exec(cut_function(train_text, 'Print_Experiment_Status'), ns)
    exec(cut_function(train_text, 'Print_Train_Status'), ns)
    settings = dict(arguments)
    settings.update(STATUS_SETTINGS)
    args = types.SimpleNamespace(**settings)
    status = io.StringIO()
    with contextlib.redirect_stdout(io.StringIO()):
        ns['Print_Experiment_Status'](args, status)
    loss_dict = {k: torch.tensor(v, dtype=torch.float32) for k, v in LOSSES.items()}
    values = {k: v.item() for k, v in loss_dict.items()}
    lines = []
    for it, ((ds_flag, extreme), sec) in enumerate(zip(FLAGS, SECONDS)):
        f = io.StringIO()
        time1 = 100.0
        ns['Print_Train_Status'](7 + it, loss_dict, ds_flag, extreme, f, time1, time1 + sec, args)
        lines.append({'iter_idx': 7 + it, 'seconds': (time1 + sec) - time1, 'ds_flag': ds_flag, 'extreme_ds_flag': extreme,
                      'text': f.getvalue()})
    assert all(ln['text'].endswith('\n') and ln['text'].count('\n') == 1 for ln in lines)

    legacy = re.sub(r' G_Reg: \S+', '', lines[0]['text'])
    log = status.getvalue() + ''.join(ln['text'] for ln in lines[:2])
    blocks = []
    for cos, lp, l1, cos_e, fid, hmap, lmark, freg in EVAL:
        blocks.append(f'\nReconstruction Quantitative Evaluation: \nCosine Similarity: {cos}\nLPIPS Score: {lp}\nL1 Score: {l1}\n'
                      f'\nEdit Quantitative Evaluation: \nEdit Cosine Similarity: {cos_e}\nFID: {fid}\nHeat Map: {hmap}\n'
                      f'Land Mark: {lmark}\nFace Regional: {freg}\n\n')
    log += blocks[0] + lines[2]['text'] + legacy + blocks[1] + '\nTotal training time: 12.345'

    ana_text = open(os.path.join(a.reference, 'Util', 'analysis_util.py')).read()
    ana = {}
    for name in ('Parse_A_Line', 'Moving_Average', 'Extract_Reconstruction_Evaluation_Score', 'Extract_Edit_Evaluation_Score'):
        exec(cut_function(ana_text, name), ana)
    parsed = []
    for ln in [x['text'] for x in lines] + [legacy]:
        try:
            parsed.append({'line': ln, 'result': list(ana['Parse_A_Line'](ln))})
        except Exception as e:      # the reference's own failure on this text is the recorded result
            parsed.append({'line': ln, 'error': type(e).__name__})
    series = [1.5, 0.5, 2.0, 4.0, 0.25, 3.0]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'log.out')
        with open(path, 'w') as f:
            f.write(log)
        rec = [list(v) for v in ana['Extract_Reconstruction_Evaluation_Score'](path)]
        edit = [list(v) for v in ana['Extract_Edit_Evaluation_Score'](path)]
    out = {'arguments': arguments, 'status_settings': settings, 'status_text': status.getvalue(), 'loss_values': values,
           'lines': lines, 'log': log, 'parse_a_line': parsed, 'moving_average': {'input': series,
                                                                                 'result': ana['Moving_Average'](series)},
           'reconstruction_scores': rec, 'edit_scores': edit}
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(a.out, os.path.getsize(a.out), 'bytes;', len(arguments), 'arguments; Parse_A_Line:',
          [p.get('result', p.get('error')) for p in parsed])


if __name__ == '__main__':
    main()
