"""Quantitative evaluation: reconstruction and editing scores (reference Evaluation/quant_eval.py:25-209).

    Compute_Face_Identity_Similarity   :25-49    cosine similarity of ArcFace features, target feature computed once
    Get_Recon_Score / Recon_Scores     :51-107   per (photo, render) pair: identity cosine, LPIPS, L1 of output vs photo
    Get_Edit_Score / Edit_Scores       :110-209  per photo and several renders: identity cosine of every output vs the
                                                 photo, face_diff_score of every output vs its render

What is different, on purpose:
  * per-sample values stay on the device and are transferred once, after the loop (the reference synchronises with the
    host three or four times per batch); `Recon_Scores` / `Edit_Scores` return them, `Get_*` their float64 means in the
    reference's tuples;
  * the metric stage of a batch (grey images for the identity network + per-sample L1) is one HIP launch
    (op/eval_scores.py) instead of ~22 elementwise ones;
  * `Edit_Scores` encodes the photo once per batch (Encode_Photo) and runs every render through
    Forward_Inference_Reanimate, and computes the photo's identity feature once per batch; the reference runs all three
    encoders for every render;
  * only the 3-encoder scheme is provided (ValueError for the 2-encoder tuple, as Reanimate_Frames);
  * the FID of the edited outputs is computed when the caller brings both an `inception_model` (Evaluation/inception.py
    with loaded weights) and `fid_stats` (the real images' statistics: a dict or the path of a pickle with `mean` and
    `cov`); neither is shipped, and an `inception_model` without `fid_stats` is refused.  The features of a batch's outputs
    go into running moments on the device (op/fid_stats.py);
  * the heat-map and landmark scores are computed when `eval_models` brings an `fa_model`: the caller's face_alignment
    model, anything with `face_detector` and `face_alignment_net` (Util/landmark_util.py; the package itself is not
    shipped).  Crops, distance and landmark decode run on their own kernels (op/landmark.py) and the per-sample values
    stay on the device; the landmarks come from the device decode, not from the package's numpy `get_preds_fromhm`.
    Without an `fa_model` those two entries of the tuple are None.
EVAL_FUSE = False (or FMGAN_NO_EVAL_FUSE=1) keeps the composite metric stage and the reference's loop structure
(Forward_Inference_3_Encoder per render, target features per call): the baseline of profiles/quant_eval.md.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from op.eval_scores import face_input
from op.fid_stats import Feature_Statistics
from op.face_region import face_region_scores
from op.landmark import heatmap_distance
from Util.landmark_util import Get_HeatMap_Landmark_PyTorch
from Util.network_util import (Encode_Photo, Forward_Inference_3_Encoder, Forward_Inference_Reanimate,
                               MODULATION_ENCODING)

from . import fid
from .calc_inception import features_of

EVAL_FUSE = os.environ.get('FMGAN_NO_EVAL_FUSE', '0') != '1'


def _gray(img):
    return face_input(img, fuse=EVAL_FUSE)[0]


def Compute_Face_Identity_Similarity(output_tensor, target_tensor, face_rec_model):
    """Cosine similarity [N] between the identity features of output and target images ([N, 3, H, W] in [-1, 1]);
    `output_tensor` may be a list of such tensors, the result is then a list.  The target's feature is computed once.
    Works on CPU tensors too (through the composite grey conversion)."""
    with torch.no_grad():
        target_feature = face_rec_model(_gray(target_tensor))
        if isinstance(output_tensor, (list, tuple)):
            return [F.cosine_similarity(face_rec_model(_gray(o)), target_feature) for o in output_tensor]
        return F.cosine_similarity(face_rec_model(_gray(output_tensor)), target_feature)


def _three_encoders(generative_model):
    if len(generative_model) != 4:
        raise ValueError('generative_model = (E_Tsr, E_W, E_W_Plus, g_ema): the 3-encoder scheme is the one this build '
                         'provides')
    return generative_model


def _same_size(what, a, b):
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f'quant_eval: {what}: {tuple(a.shape)} against {tuple(b.shape)}: the scores compare images '
                         f'pixel by pixel; nothing is resampled')


def _mean(t):
    return np.mean(t.detach().to('cpu', torch.float64).numpy())


def Recon_Scores(eval_loader, device, generative_model, eval_models, info_print=False, **kwargs):
    """Per-sample reconstruction scores, in loader order, as device tensors: dict(cos, lpips, l1).  eval_loader yields
    (photo, render) batches (ragged last batch allowed); generative_model = (E_Tsr, E_W, E_W_Plus, g_ema);
    eval_models = (face_rec_model, percept_loss); kwargs go to Forward_Inference_3_Encoder (tsr_encode, sliced_layer,
    use_tanh).  Nothing synchronises with the host."""
    E_Tsr, E_W, E_W_Plus, g_ema = _three_encoders(generative_model)
    face_rec_model, percept_loss = eval_models
    cos, lpips, l1 = [], [], []
    with torch.no_grad():
        for idx, (p_input, r_input) in enumerate(eval_loader):
            if info_print:
                print('Batch: ' + str(idx))
            p_input, r_input = p_input.to(device), r_input.to(device)
            g_output = Forward_Inference_3_Encoder(p_input, r_input, E_Tsr, E_W, E_W_Plus, g_ema, **kwargs)
            _same_size('output and photo', g_output, p_input)
            if EVAL_FUSE:
                gray_g, gray_p, l1_score = face_input(g_output, p_input, want_gray_b=True, want_l1=True)
                cos.append(F.cosine_similarity(face_rec_model(gray_g), face_rec_model(gray_p)))
            else:
                cos.append(Compute_Face_Identity_Similarity(g_output, p_input, face_rec_model))
                l1_score = torch.mean(torch.abs(g_output - p_input), dim=(1, 2, 3))
            lpips.append(percept_loss(g_output, p_input).reshape(-1))
            l1.append(l1_score)
    if not cos:
        raise ValueError('Recon_Scores: the loader yielded no batch')
    return {'cos': torch.cat(cos), 'lpips': torch.cat(lpips), 'l1': torch.cat(l1)}


def Get_Recon_Score(eval_loader, device, generative_model, eval_models, info_print=False, **kwargs):
    """(mean cosine similarity, mean LPIPS, mean L1) over the loader, float64 means of the per-sample values: the
    reference's 3-tuple."""
    s = Recon_Scores(eval_loader, device, generative_model, eval_models, info_print, **kwargs)
    if info_print:
        print('Cosine Similarity Len: ' + str(len(s['cos'])) + ' LPIPS Len: ' + str(len(s['lpips'])) + ' L1 Len: '
              + str(len(s['l1'])))
    return _mean(s['cos']), _mean(s['lpips']), _mean(s['l1'])


class _NoiseArgs:
    """g_ema with the noise arguments pinned, for Forward_Inference_3_Encoder (which passes none)."""

    def __init__(self, g_ema, noise, randomize_noise):
        self.module = getattr(g_ema, 'module', g_ema)
        self._call, self._kw = g_ema, dict(noise=noise, randomize_noise=randomize_noise)

    def __call__(self, **kw):
        return self._call(**self._kw, **kw)


def Edit_Scores(eval_loader, device, generative_model, eval_models, info_print=False, tsr_encode=MODULATION_ENCODING[1],
                sliced_layer=None, use_tanh=False, noise=None, randomize_noise=True, fid_stats=None):
    """Per-sample editing scores as device tensors: dict(cos, face_diff), and with an fa_model also hmap (sum of squared
    heat-map differences of render and output) and lmark (mean squared landmark difference in the image's frame).
    eval_loader yields [photo, render_1, ..., render_n] batches; eval_models = (face_rec_model, inception_model,
    fa_model), fa_model None or the caller's alignment model (Util/landmark_util.py).  Order of every list: batch by
    batch, render-major within a batch (all samples of render 1, then render 2, ...), as the reference appends them.  noise / randomize_noise go to the generator (its own defaults when not given).  With an inception_model
    and fid_stats (the real statistics) the dict also holds `fid_state`: the Feature_Statistics of every output's features
    (a batch's outputs concatenated, one pass through the model)."""
    E_Tsr, E_W, E_W_Plus, g_ema = _three_encoders(generative_model)
    face_rec_model, inception_model, fa_model = eval_models
    if inception_model is not None and fid_stats is None:
        raise ValueError('Edit_Scores: inception_model without fid_stats: FID needs Inception weights and the FFHQ '
                         'statistics file, which are not shipped; pass both, or inception_model=None')
    if fa_model is not None and not (hasattr(fa_model, 'face_detector') and hasattr(fa_model, 'face_alignment_net')):
        raise ValueError('Edit_Scores: fa_model must be None or a face_alignment.FaceAlignment (anything with '
                         '`face_detector` and `face_alignment_net`): the heat-map and landmark scores run the caller\'s '
                         'two networks')
    if tsr_encode not in MODULATION_ENCODING:
        raise ValueError(f'tsr_encode must be one of {MODULATION_ENCODING}')
    cos, face_diff, hmap, lmark, fid_state = [], [], [], [], None
    with torch.no_grad():
        for idx, img_tensor_list in enumerate(eval_loader):
            if info_print:
                print('Batch: ' + str(idx))
            p_input = img_tensor_list[0].to(device)
            renders = [r.to(device) for r in img_tensor_list[1:]]
            outputs = []
            if EVAL_FUSE:
                code = Encode_Photo(p_input, E_Tsr, E_W_Plus, tsr_encode)
                target_feature = face_rec_model(_gray(p_input))
                for r_input in renders:
                    g_output = Forward_Inference_Reanimate(code, r_input, E_Tsr, E_W, g_ema, tsr_encode, sliced_layer,
                                                           use_tanh, noise, randomize_noise)
                    _same_size('render and output', r_input, g_output)
                    face_diff.append(face_region_scores(r_input, g_output))
                    cos.append(F.cosine_similarity(face_rec_model(_gray(g_output)), target_feature))
                    outputs.append(g_output)
            else:
                g = g_ema if noise is None and randomize_noise else _NoiseArgs(g_ema, noise, randomize_noise)
                g_output_list = []
                for r_input in renders:
                    g_output = Forward_Inference_3_Encoder(p_input, r_input, E_Tsr, E_W, E_W_Plus, g, tsr_encode,
                                                           sliced_layer, use_tanh)
                    _same_size('render and output', r_input, g_output)
                    g_output_list.append(g_output)
                    face_diff.append(face_region_scores(r_input, g_output))
                cos += Compute_Face_Identity_Similarity(g_output_list, p_input, face_rec_model)
                outputs = g_output_list
            if fa_model is not None:
                for r_input, g_output in zip(renders, outputs):
                    heatmap_g, landmark_g = Get_HeatMap_Landmark_PyTorch(g_output, fa_model, device)
                    heatmap_r, landmark_r = Get_HeatMap_Landmark_PyTorch(r_input, fa_model, device)
                    hmap.append(heatmap_distance(heatmap_r, heatmap_g))
                    lmark.append(torch.mean(torch.square(landmark_r - landmark_g), dim=(1, 2)))
            if inception_model is not None and outputs:
                feat = features_of(inception_model, torch.cat(outputs), fid.FID_FUSE)
                if fid_state is None:
                    fid_state = Feature_Statistics(feat.shape[1], feat.device, fuse=fid.FID_FUSE)
                fid_state.update(feat)
    if not cos:
        raise ValueError('Edit_Scores: the loader yielded no render')
    scores = {'cos': torch.cat(cos), 'face_diff': torch.cat(face_diff)}
    if fa_model is not None:
        scores['hmap'], scores['lmark'] = torch.cat(hmap), torch.cat(lmark)
    if fid_state is not None:
        scores['fid_state'] = fid_state
    return scores


def Get_Edit_Score(eval_loader, device, generative_model, eval_models, info_print=False, **kwargs):
    """(mean cosine similarity, fid, heat-map score, landmark score, mean face difference): the reference's 5-tuple, with
    None for the scores not computed: the heat-map and landmark scores unless eval_models brings an fa_model, the FID
    unless it brings an inception_model and `fid_stats` (the real images' statistics: a dict or a pickle path with `mean` / `cov`) is given."""
    real = None
    if eval_models[1] is not None and kwargs.get('fid_stats') is not None:
        real = fid.load_real_stats(kwargs['fid_stats'])          # before the loop: a wrong path fails at once
    s = Edit_Scores(eval_loader, device, generative_model, eval_models, info_print, **kwargs)
    if info_print:
        print('Cosine Similarity Len: ' + str(len(s['cos'])) + ' FaceDiff Len: ' + str(len(s['face_diff'])))
    fid_score = None
    if 'fid_state' in s:
        fid_score = fid.calc_fid(*s['fid_state'].finish(), *real)
    hmap_score = _mean(s['hmap']) if 'hmap' in s else None
    lmark_score = _mean(s['lmark']) if 'lmark' in s else None
    return _mean(s['cos']), fid_score, hmap_score, lmark_score, _mean(s['face_diff'])
