"""One training iteration of the 3-encoder scheme on the MI355X path, data-parallel as one process per GPU.

The reference's train_3_encoder.py cannot be imported (a duplicated tail after main() is a SyntaxError) and
drives its GPUs through single-process nn.DataParallel.  This module re-states the step functions `train()` calls
(train_3_encoder.py:756-828), with the reference's names, argument order and arithmetic:

    D_Loss_BackProp   :448-477   logistic D loss on (reference image, generated image), G/encoders frozen
    D_Reg_BackProp    :479-493   R1 on the reference images every d_reg_every iterations (second order)
    G_Loss_BackProp   :495-558   non-saturating G loss + weighted reconstruction losses (+ the face-regional loss
                                 on dual-supervision batches), G + encoders trained
    G_Reg_BackProp    :561-596   path-length regulariser every g_reg_every iterations on batch / shrink (second order)
    accumulate        :195-200   EMA of G into g_ema            Optimizer_Initilization :399-444
    Trainer.train_iteration :777-822   the schedule of train(): one dual-supervision iteration in every ds_freq, one
                                 extreme-pose iteration in every ex_ds_freq of those, D_edit (if given) as their D

What is different, on purpose:
  * gradients are averaged over ranks (RCCL all-reduce: DDP buckets, or Miscellaneous.distributed.gather_grad) instead
    of DataParallel's reduce-to-device-0; the path-length mean is taken over the GLOBAL batch through a differentiable
    all-reduce, as DataParallel's gather made it;
  * the generated image of the D step comes from the no_grad inference schedule (fused epilogues, side streams): its
    producers are frozen there (requires_grad(G, False), :453-457), so values are identical and no graph is kept;
  * the LPIPS and ArcFace terms (:529,:535) are computed when `lpips_model` / `face_rec_model` are passed, with the
    reference's weights and arithmetic; their pretrained weights are not available offline, so
    Module_Fix_Setup builds the two networks (lpips/, Util/arcface_pytorch/) with their own initialisation — the cost of
    the iteration is that of the reference's, the loss VALUES are not.  The face-regional term (:544-547, weights
    rec/ds/ep = 0/20/100, train_3_encoder_hyperparams.py:69-71) is plain tensor arithmetic and runs on its own HIP
    kernel (op/face_region.py); it needs renders of the output's size, so at 1024^2 outputs from 256^2 renders a
    dual-supervision iteration raises ValueError (the reference broadcasts there; resampling is not provided).  The
    landmark heat-map term (:538-542) is computed when `fa_model` (the caller's face_alignment model: detector and
    alignment network) is passed and iter_idx > args.hmap_iter_thres, with weight args.hmap_loss_lambda (0 and inf in
    the reference's setting, train_3_encoder_hyperparams.py:66-68); its crops and distance run on their own HIP kernels
    (op/landmark.py).  `extra_losses` takes any further (name, weight, fn(output, reference) -> scalar) terms.
  * the schedule is opt-in: Trainer.step(...) without flags is a reconstruction iteration, exactly as before;
    Trainer.train_iteration(...) draws the flags and the batch as train() does.

The program around them is at the end of the file: Args_Parsing, Print_Experiment_Status,
Module_To_Train_Setup, Training_Setup, Print_Train_Status, train() and main() (:43-187, :311-364, :599-665, :756-875).
train() adds two launches per iteration and no host synchronisation: the loss values go through op.loss_log.LossLedger
(one launch per iteration, read back every args.log_flush iterations) instead of nine .item() per iteration, and with
args.ema_fuse the EMA is one launch (op.ema.EmaPlan) instead of two per parameter.
"""
import argparse
import contextlib
import os
import types

import numpy as np
import torch
from torch import nn, optim

import dataset
from Miscellaneous import distributed as D_
from op import _native
from Util.network_util import CO_MODULATION_MODE, Forward_Inference_3_Encoder, MODULATION_ENCODING
from Util.training_util import (Face_Identity_Loss, Face_Regional_Loss, Heat_Map_Loss, L1_Loss, LPIPS_Loss, accumulate,
                                accumulate_fused, d_logistic_loss, d_r1_loss, g_nonsaturating_loss, requires_grad)


# Default of --bf16_io / args.bf16_io: the 16-bit activation kernels under --precision bf16.  On, because the bf16
# training step at 1024^2 is faster with them by far more than its run-to-run spread (profiles/act16.md).
BF16_IO_DEFAULT = True


def default_args(**over):
    """The fields of `args` the step functions and Sample_Eval_Save_Ckpt read, with train_3_encoder_hyperparams.py:23-79
    defaults."""
    a = types.SimpleNamespace(
        tsr_encode=MODULATION_ENCODING[0], w_plus_sliced_layer=None, use_tanh=False,
        tsr_train=True, w_train=True, w_plus_train=True,
        lr=0.001, rec_batch=16, r1=10, d_reg_every=16, use_g_reg=True, g_reg_every=4, generator_path_reg_weight=2,
        path_reg_batch_shrink=2, l1_loss_lambda=3, lpips_loss_lambda=3, ep_lpips_l1_weight_shrink=10,
        face_id_loss_lambda=30, face_id_loss_type='MSE', grad_sync='ddp',
        hmap_loss_lambda=0, hmap_iter_thres=np.inf,                                                # :66-68
        ds_freq=2, ex_ds_freq=3, rec_face_reg_loss_lambda=0, ds_face_reg_loss_lambda=20, ep_face_reg_loss_lambda=100,
        val_sample_freq=1000, model_save_freq=10000, n_real_eval_faces=2, n_syn_eval_faces=2,      # :73-79
        val_sample_tile=256,        # this build's: side of the sample sheet's tiles (the output's size for a Generator below 256)
        # what Dataset_DataLoader_Setup reads (:20-23, :47-52, :74-76); the reference's defaults are its authors' folders
        size=256, synface_dir=None, extreme_pose_dir=None, ffhq_train_img_dir=None, quant_eval_img_dir=None,
        visual_real_img_dir=None, rec_dataset_type='FFHQ', ds_dataset_type='Synthetic', ds_batch=16,
        quant_eval_batch_size=64,
        num_workers=8,              # this build's: worker processes per DataLoader of the non-resident path (at most 16)
        bank_cache_dir=None)        # this build's: folder the decoded banks are kept in as .npy (None: decode every run)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _local(net):
    """The network without DDP's gradient hooks, for calls in which all of its parameters are frozen (a DDP forward
    with nothing to reduce would still arm the reducer); any other wrapper is called as given."""
    return net.module if isinstance(net, nn.parallel.DistributedDataParallel) else net


def _sync_grads(args, nets):
    """Explicit gradient averaging for Replica-wrapped networks (grad_sync='flat'); DDP does it inside backward."""
    if getattr(args, 'grad_sync', 'ddp') != 'flat' or D_.get_world_size() == 1:
        return
    params = [p for n in nets for p in n.parameters() if p.requires_grad]
    D_.gather_grad(params, algorithm=getattr(args, 'grad_algorithm', 'reduce_scatter'))


def Module_Fix_Setup(args, device):
    """The frozen loss networks of train_3_encoder.py:366-396 that can be built offline: LPIPS (net-lin / VGG16) and the
    ArcFace identity network (resnet_face18, use_se=False), eval mode, no parameter gradients.  Returns
    (lpips_model, face_rec_model).  The VGG trunk runs channels_last: MIOpen's fp32 implicit-GEMM kernels are NHWC-native
    (same finding as for the pSp encoder)."""
    import lpips
    from Util.arcface_pytorch.resnet_face_recognition import resnet_face18
    lpips_model = lpips.PerceptualLoss(model='net-lin', net='vgg').to(device)
    face_rec_model = resnet_face18(use_se=False).to(device)
    requires_grad(face_rec_model, False)
    face_rec_model.eval()
    if torch.device(device).type == 'cuda' and getattr(args, 'loss_nets_channels_last', True):
        lpips_model = lpips_model.to(memory_format=torch.channels_last)
        face_rec_model = face_rec_model.to(memory_format=torch.channels_last)
    return lpips_model, face_rec_model


class sample_data:
    """The endless batch stream of train() (train_3_encoder.py:203-206): `while True: for batch in loader: yield batch`.
    An object, not a generator, so that a loader that assembles training triples itself (dataset.BankLoader) keeps its
    training_batch() behind it, with the same roll-over into the next epoch; iter(loader) is first called when the
    first batch is asked for, as a generator would."""

    def __init__(self, loader):
        self.loader = loader
        self._it = None

    def __iter__(self):
        return self

    def _rolling(self, take):
        if self._it is None:
            self._it = iter(self.loader)
        try:
            return take()
        except StopIteration:
            self._it = iter(self.loader)
            try:
                return take()
            except StopIteration:
                raise RuntimeError('sample_data: the loader yields no batch') from None

    def __next__(self):
        return self._rolling(lambda: next(self._it))

    def __getattr__(self, name):
        # only where the loader has it: dataset.Data_Loading asks with hasattr
        if name == 'training_batch' and hasattr(self.__dict__.get('loader'), 'training_batch'):
            return lambda **kw: self._rolling(lambda: self.loader.training_batch(**kw))
        raise AttributeError(name)


def Visual_Evaluation_Setup(args, synface_dataset, extreme_pose_dataset, transform, device=None):
    """The sample sets of the visual validation (train_3_encoder.py:213-223): synthetic, extreme-pose, then real."""
    import os
    from Evaluation.visual_eval import Get_Real_Img_Val_Sample, Get_Syn_Img_Val_Sample
    device = device if device is not None else args.device
    real_img_list = [os.path.join(args.visual_real_img_dir, f) for f in os.listdir(args.visual_real_img_dir)]
    real_img_eval_samples = Get_Real_Img_Val_Sample(real_img_list, transform, args.n_real_eval_faces, device)
    syn_img_eval_samples = Get_Syn_Img_Val_Sample(synface_dataset, args.n_syn_eval_faces, device)
    ep_img_eval_samples = Get_Syn_Img_Val_Sample(extreme_pose_dataset, args.n_syn_eval_faces, device)
    return syn_img_eval_samples + ep_img_eval_samples + real_img_eval_samples


N_IMG_PER_ID = 7        # images per identity of the synthetic trees (train_3_encoder.py:271,277)


def Dataset_DataLoader_Setup(args, device=None, resident=True):
    """Datasets and loaders of train() (train_3_encoder.py:226-308), the reference's 9-tuple:
    (transform, synface_dataset, extreme_pose_dataset, rec / ds / ep / pure-FFHQ training streams, rec_eval_loader,
    edit_eval_loader), with its batch sizes, shuffling and samplers.

    resident=True: every dataset is decoded once into uint8 banks on `device` (dataset.Resident; kept under
    args.bank_cache_dir when set; folders that several datasets read are decoded once), the loaders are
    dataset.BankLoaders and the two datasets returned are the Residents, which index like the datasets they hold.
    resident=False: torch DataLoaders over the datasets with dataset.Transform and args.num_workers workers (at most
    16).  A folder argument that is None leaves its loaders None.  With more than one rank each rank keeps the whole
    bank and its samplers draw from torch.Generator().manual_seed(args.seed + rank); a single rank draws from torch's
    global generator, as the reference does."""
    import os
    from torch.utils import data
    size = args.size
    transform = dataset.Transform(size)
    device = torch.device(device if device is not None else getattr(args, 'device', 'cuda'))
    generator = None
    if D_.get_world_size() > 1:
        generator = torch.Generator()
        generator.manual_seed(int(getattr(args, 'seed', 0)) + D_.get_rank())
    workers = max(0, min(int(getattr(args, 'num_workers', 8)), 16))
    share = {}

    def held(ds, name):
        if not resident:
            return ds
        cache = getattr(args, 'bank_cache_dir', None)
        if cache is not None:
            os.makedirs(cache, exist_ok=True)
            cache = os.path.join(cache, f'{name}_{size}')
        return dataset.Resident(ds, size, device, cache=cache, share=share, workers=max(1, workers))

    def loader(ds, batch_size, shuffle=False, sampler=None):
        if ds is None:
            return None
        if not resident:
            return data.DataLoader(ds, batch_size=batch_size, shuffle=shuffle if sampler is None else None,
                                   sampler=sampler, num_workers=workers, generator=generator)
        if sampler is None:
            sampler = data.RandomSampler(ds, generator=generator) if shuffle else data.SequentialSampler(ds)
        return dataset.BankLoader(ds, batch_size, sampler)

    def stream(ld):
        return None if ld is None else sample_data(ld)

    def sub(root, name):
        return None if root is None else os.path.join(root, name)

    train_dir, eval_dir = args.ffhq_train_img_dir, args.quant_eval_img_dir
    if train_dir is None and 'FFHQ' in (args.rec_dataset_type, args.ds_dataset_type):
        raise ValueError('Dataset_DataLoader_Setup: an FFHQ dataset type needs args.ffhq_train_img_dir')
    synface_dataset = held(dataset.Synthetic_Dataset(args.synface_dir, transform), 'synface')
    extreme_pose_dataset = held(dataset.Synthetic_Dataset(args.extreme_pose_dir, transform), 'extreme_pose')

    if args.rec_dataset_type == 'FFHQ':
        recon_dataset = held(dataset.FFHQ_Dataset_Reconstruction(sub(train_dir, 'img'), sub(train_dir, 'render_img'),
                                                                 transform), 'ffhq_train_rec')
    elif args.rec_dataset_type == 'Synthetic':
        recon_dataset = synface_dataset
    else:
        raise ValueError(f'rec_dataset_type {args.rec_dataset_type!r}: \'FFHQ\' or \'Synthetic\'')
    rec_train_loader = loader(recon_dataset, args.rec_batch, shuffle=True)

    if args.ds_dataset_type == 'FFHQ':
        edit_train = held(dataset.FFHQ_Dataset_Editing(sub(train_dir, 'img'), sub(train_dir, 'edit_render_img'), transform,
                                                       train=True, render_image_folder=sub(train_dir, 'render_img')),
                          'ffhq_train_edit')
        ds_train_loader = loader(edit_train, args.ds_batch // 2, shuffle=True)
    elif args.ds_dataset_type == 'Synthetic':
        ds_sampler = dataset.DualSupervisionSampler(synface_dataset, N_IMG_PER_ID, generator=generator)
        ds_train_loader = loader(synface_dataset, args.ds_batch, sampler=ds_sampler)
    else:
        raise ValueError(f'ds_dataset_type {args.ds_dataset_type!r}: \'FFHQ\' or \'Synthetic\'')
    ep_sampler = dataset.ExtremePoseDualSupervisionSampler(extreme_pose_dataset, N_IMG_PER_ID, generator=generator)
    ep_train_loader = loader(extreme_pose_dataset, args.ds_batch * 2, sampler=ep_sampler)

    pure_ffhq_loader = None
    if train_dir is not None:
        pure_ffhq_loader = loader(held(dataset.FFHQ_Dataset(sub(train_dir, 'img'), transform), 'ffhq_train'),
                                  args.ds_batch // 2, shuffle=True)
    rec_eval_loader = edit_eval_loader = None
    if eval_dir is not None:
        rec_eval = held(dataset.FFHQ_Dataset_Reconstruction(sub(eval_dir, 'img'), sub(eval_dir, 'render_img'), transform),
                        'ffhq_eval_rec')
        rec_eval_loader = loader(rec_eval, args.quant_eval_batch_size)
        edit_eval = held(dataset.FFHQ_Dataset_Editing(sub(eval_dir, 'img'), sub(eval_dir, 'edit_render_img'), transform,
                                                      train=False), 'ffhq_eval_edit')
        edit_eval_loader = loader(edit_eval, args.quant_eval_batch_size // 4)
    return (transform, synface_dataset, extreme_pose_dataset, stream(rec_train_loader), stream(ds_train_loader),
            stream(ep_train_loader), stream(pure_ffhq_loader), rec_eval_loader, edit_eval_loader)


def Optimizer_Initilization(args, G, E_Tsr, E_W, E_W_Plus, D, D_edit=None, ckpt=None):
    """Adam with the lazy-regularisation learning-rate / beta correction (train_3_encoder.py:399-444)."""
    g_reg_ratio = args.g_reg_every / (args.g_reg_every + 1)
    d_reg_ratio = args.d_reg_every / (args.d_reg_every + 1)
    g_enc_params = list(G.parameters())
    if args.tsr_train:
        g_enc_params += list(E_Tsr.parameters())
    if args.w_train:
        g_enc_params += list(E_W.parameters())
    if args.w_plus_train:
        g_enc_params += list(E_W_Plus.parameters())
    g_enc_optim = optim.Adam(g_enc_params, lr=args.lr * g_reg_ratio, betas=(0 ** g_reg_ratio, 0.99 ** g_reg_ratio))
    d_optim = optim.Adam(D.parameters(), lr=args.lr * d_reg_ratio, betas=(0 ** d_reg_ratio, 0.99 ** d_reg_ratio))
    d_edit_optim = None
    if D_edit is not None:
        d_edit_optim = optim.Adam(D_edit.parameters(), lr=args.lr * d_reg_ratio,
                                  betas=(0 ** d_reg_ratio, 0.99 ** d_reg_ratio))
    if ckpt is not None and getattr(args, 'load_train_state', False):
        g_enc_optim.load_state_dict(ckpt['g_enc_optim'])
        d_optim.load_state_dict(ckpt['d_optim'])
        if 'd_edit_optim' in ckpt and d_edit_optim is not None:
            d_edit_optim.load_state_dict(ckpt['d_edit_optim'])
    return g_enc_optim, d_optim, d_edit_optim


def D_Loss_BackProp(G, E_Tsr, E_W, E_W_Plus, D, g_input, r_input, g_ref, args, loss_dict, d_optim, d_type='D'):
    """Update D on the logistic GAN loss (train_3_encoder.py:448-477)."""
    requires_grad(G, False)
    requires_grad(E_Tsr, False)
    requires_grad(E_W, False)
    requires_grad(E_W_Plus, False)
    requires_grad(D, True)
    with torch.no_grad():       # every producer is frozen: same values, inference schedule, no graph
        g_output = Forward_Inference_3_Encoder(g_input, r_input, _local(E_Tsr), _local(E_W), _local(E_W_Plus), G,
                                               args.tsr_encode, args.w_plus_sliced_layer, args.use_tanh)
    out_pred = D(g_output)
    ref_pred = D(g_ref)
    d_loss = d_logistic_loss(ref_pred, out_pred)
    if d_type == 'D':
        loss_dict['d'] = d_loss
        loss_dict['ref_score'] = ref_pred.mean()
        loss_dict['out_score'] = out_pred.mean()
    else:
        loss_dict['d_edit'] = d_loss
        loss_dict['ref_score_ffhq'] = ref_pred.mean()
        loss_dict['out_score_ffhq'] = out_pred.mean()
    D.zero_grad()
    d_loss.backward()
    _sync_grads(args, [D])
    if d_optim is not None:
        d_optim.step()


def D_Reg_BackProp(real_img, D, args, d_optim):
    """Update D on the R1 penalty (train_3_encoder.py:479-493); returns the unweighted penalty."""
    real_img = real_img.detach().requires_grad_(True)
    real_pred = D(real_img)
    r1_loss = d_r1_loss(real_pred, real_img)
    D.zero_grad()
    (args.r1 / 2 * r1_loss * args.d_reg_every + 0 * real_pred[0]).backward()
    _sync_grads(args, [D])
    if d_optim is not None:
        d_optim.step()
    return r1_loss


def _trained(args, G, E_Tsr, E_W, E_W_Plus):
    nets = [G]
    if args.tsr_train:
        nets.append(E_Tsr)
    if args.w_train:
        nets.append(E_W)
    if args.w_plus_train:
        nets.append(E_W_Plus)
    return nets


def face_reg_lambda(args, ds_flag, extreme_ds_flag):
    """Weight of the face-regional term for this batch (train_3_encoder.py:521-526)."""
    if not ds_flag:
        return args.rec_face_reg_loss_lambda
    if not extreme_ds_flag:
        return args.ds_face_reg_loss_lambda
    return args.ep_face_reg_loss_lambda


def G_Loss_BackProp(G, E_Tsr, E_W, E_W_Plus, D, g_input, r_input, g_ref, args, loss_dict, g_enc_optim,
                    lpips_model=None, face_rec_model=None, fa_model=None, iter_idx=0, extreme_ds_flag=False,
                    ds_flag=False, extra_losses=()):
    """Update G and the encoders on the adversarial + reconstruction losses (train_3_encoder.py:495-558; the
    reference's argument order).  lpips_model / face_rec_model = None leaves that term out.  The heat-map term is
    added when fa_model is given and iter_idx > args.hmap_iter_thres; otherwise loss_dict['hmap'] is a zero, as in the
    reference (:538-542).  The face-regional term is added last, with face_reg_lambda(args, ds_flag,
    extreme_ds_flag); at weight 0 (reconstruction batches) it is not computed and loss_dict['face_reg'] is a zero,
    which is what the reference's 0 * term contributes."""
    requires_grad(G, True)
    requires_grad(E_Tsr, args.tsr_train)
    requires_grad(E_W, args.w_train)
    requires_grad(E_W_Plus, args.w_plus_train)
    requires_grad(D, False)
    g_output = Forward_Inference_3_Encoder(g_input, r_input, E_Tsr, E_W, E_W_Plus, G, args.tsr_encode,
                                           args.w_plus_sliced_layer, args.use_tanh)
    out_pred = _local(D)(g_output)            # D is frozen here: nothing of it to synchronise
    g_loss = g_nonsaturating_loss(out_pred)
    loss_dict['g'] = g_loss
    shrink = args.ep_lpips_l1_weight_shrink if extreme_ds_flag else 1        # :517-519
    face_id_reference = g_input if extreme_ds_flag else g_ref
    l1_loss = args.l1_loss_lambda / shrink * L1_Loss(g_output, g_ref)
    loss_dict['l1'] = l1_loss
    total_loss = g_loss + l1_loss
    if lpips_model is not None:
        loss_dict['lpips'] = args.lpips_loss_lambda / shrink * LPIPS_Loss(g_output, g_ref, lpips_model)
        total_loss = total_loss + loss_dict['lpips']
    if face_rec_model is not None:
        loss_dict['face_id'] = args.face_id_loss_lambda * Face_Identity_Loss(g_output, face_id_reference, face_rec_model,
                                                                              args.face_id_loss_type)
        total_loss = total_loss + loss_dict['face_id']
    for name, weight, fn in extra_losses:
        loss_dict[name] = weight * fn(g_output, g_ref)
        total_loss = total_loss + loss_dict[name]
    if fa_model is not None and iter_idx > getattr(args, 'hmap_iter_thres', np.inf):
        loss_dict['hmap'] = getattr(args, 'hmap_loss_lambda', 0) * Heat_Map_Loss(g_output, r_input, fa_model)
        total_loss = total_loss + loss_dict['hmap']
    else:
        loss_dict['hmap'] = torch.zeros((), device=g_output.device)
    face_reg_loss_lambda = face_reg_lambda(args, ds_flag, extreme_ds_flag)
    if face_reg_loss_lambda:
        loss_dict['face_reg'] = face_reg_loss_lambda * Face_Regional_Loss(r_input, g_output)
        total_loss = total_loss + loss_dict['face_reg']
    else:
        loss_dict['face_reg'] = torch.zeros((), device=g_output.device)
    nets = _trained(args, G, E_Tsr, E_W, E_W_Plus)
    for n in nets:
        n.zero_grad()
    total_loss.backward()
    _sync_grads(args, nets)
    if g_enc_optim is not None:
        g_enc_optim.step()


def _global_mean(x):
    """Mean over the samples of ALL ranks, differentiable (backward = the same all-reduce on the gradient)."""
    m = x.mean()
    if D_.get_world_size() == 1:
        return m
    from torch.distributed.nn import functional as dist_fn
    return dist_fn.all_reduce(m) / D_.get_world_size()


def G_Reg_BackProp(G, E_Tsr, E_W, E_W_Plus, g_input, r_input, args, mean_path_length, g_enc_optim, choice=None):
    """Update G and the encoders on the path-length regulariser (train_3_encoder.py:561-596).
    `choice`: indices of the batch/shrink samples (the reference draws them with np.random.choice)."""
    batch = g_input.shape[0]
    path_batch_size = max(1, batch // args.path_reg_batch_shrink)
    if choice is None:
        choice = np.random.choice(range(batch), size=path_batch_size, replace=False)
    idx = torch.as_tensor(np.asarray(choice), device=g_input.device, dtype=torch.long)
    g_input_reg, r_input_reg = g_input.index_select(0, idx), r_input.index_select(0, idx)
    g_output, path_lengths = Forward_Inference_3_Encoder(g_input_reg, r_input_reg, E_Tsr, E_W, E_W_Plus, G,
                                                         args.tsr_encode, args.w_plus_sliced_layer, args.use_tanh,
                                                         PPL_regularize=True)
    decay = 0.01
    path_mean = mean_path_length + decay * (_global_mean(path_lengths) - mean_path_length)
    path_loss = (path_lengths - path_mean).pow(2).mean()
    mean_path_length = path_mean.detach()
    nets = _trained(args, G, E_Tsr, E_W, E_W_Plus)
    for n in nets:
        n.zero_grad()
    weighted_path_loss = args.generator_path_reg_weight * args.g_reg_every * path_loss
    if args.path_reg_batch_shrink:
        weighted_path_loss = weighted_path_loss + 0 * g_output[0, 0, 0, 0]
    weighted_path_loss.backward()
    _sync_grads(args, nets)
    if g_enc_optim is not None:
        g_enc_optim.step()
    return path_loss, path_lengths, mean_path_length


def training_precision(args):
    """(precision, bf16_io) of a Trainer with these settings: args.precision ('fp32' when the field is absent, as in
    default_args()) and whether the 16-bit activation kernels are on — args.bf16_io under 'bf16', unless
    FMGAN_NO_BF16_IO=1 (read at every step, like the other FMGAN_NO_* switches)."""
    precision = getattr(args, 'precision', 'fp32')
    if precision not in ('fp32', 'bf16'):
        raise ValueError(f"args.precision must be 'fp32' or 'bf16', got {precision!r}")
    io = (precision == 'bf16' and bool(getattr(args, 'bf16_io', BF16_IO_DEFAULT))
          and os.environ.get('FMGAN_NO_BF16_IO') != '1')
    return precision, io


def precision_context(args):
    """What Trainer.step runs inside.  'fp32': nothing.  'bf16': torch.autocast(bfloat16) + the bf16 MFMA contraction of
    the modulated convolutions (+ 16-bit activations in HBM with bf16_io) around the forward, backward and optimiser
    steps of the iteration; parameters, the gradients Adam applies, its moments and the EMA stay fp32.  A labelled
    reduced-precision extension, never the parity path; sample(), evaluate() and checkpoints do not enter it."""
    precision, io = training_precision(args)
    stack = contextlib.ExitStack()
    if precision == 'bf16':
        stack.enter_context(torch.autocast('cuda', dtype=torch.bfloat16))
        stack.enter_context(_native.modconv_precision('bf16'))
        stack.enter_context(_native.activation_io('16' if io else 'fp32'))
    return stack


class Trainer:
    """State of `train()` (train_3_encoder.py:756-828) for one rank: wrapped networks, g_ema, optimisers, counters.

    nets: dict with G, E_Tsr, E_W, E_W_Plus, D and optionally D_edit, the editing discriminator of the
    dual-supervision iterations (bare modules on this rank's device; BatchNorm of the encoders in eval mode, SURVEY
    F13).  grad_sync: 'ddp' wraps them in DistributedDataParallel, 'flat' in Replica + gather_grad."""

    def __init__(self, nets, args, device=None, g_ema=None, lpips_model=None, face_rec_model=None, fa_model=None):
        import copy
        self.args = args
        self.lpips_model, self.face_rec_model, self.fa_model = lpips_model, face_rec_model, fa_model
        ddp = getattr(args, 'grad_sync', 'ddp') == 'ddp'
        self.bare = dict(nets)
        self.g_ema = g_ema if g_ema is not None else copy.deepcopy(nets['G']).eval().requires_grad_(False)
        for m in nets.values():
            m.requires_grad_(True)
        # unused parameters exist in G (mapping network, constant input) and — when only some W+ columns are
        # co-modulated — in the pSp encoder's style heads of the other columns
        unused = {'G': True, 'E_W_Plus': args.w_plus_sliced_layer is not None}
        self.nets = {k: D_.data_parallel(m, device, overlap=ddp, find_unused_parameters=unused.get(k, False))
                     for k, m in nets.items()}
        self.g_enc_optim, self.d_optim, self.d_edit_optim = Optimizer_Initilization(
            args, self.bare['G'], self.bare['E_Tsr'], self.bare['E_W'], self.bare['E_W_Plus'], self.bare['D'],
            self.bare.get('D_edit'))
        self.device = device
        self.accum = 0.5 ** (32 / (10 * 1000))
        self.mean_path_length = 0
        self.iter_idx = 0
        self.ds_count = 0
        self.loss_dict = {'r1': torch.zeros((), device=device), 'g_reg': torch.zeros((), device=device)}
        self.ema_plan = None        # op.ema.EmaPlan of (g_ema, G) once step() has run with args.ema_fuse; validates itself

    def ds_flags(self):
        """(ds_flag, extreme_ds_flag) of the coming iteration, self.iter_idx (train_3_encoder.py:780-786): every
        ds_freq-th iteration is a dual-supervision one, and every ex_ds_freq-th of those uses the extreme-pose batch;
        ds_count counts the dual-supervision iterations."""
        a = self.args
        if self.iter_idx % a.ds_freq != a.ds_freq - 1:
            return False, False
        extreme_ds_flag = self.ds_count % a.ex_ds_freq == a.ex_ds_freq - 1
        self.ds_count += 1
        return True, extreme_ds_flag

    def discriminator(self, ds_flag=False):
        """(wrapped network, optimiser) on the D side of an iteration: D_edit on dual-supervision batches when it was
        given (train_3_encoder.py:788-796), D otherwise."""
        if ds_flag and 'D_edit' in self.nets:
            return self.nets['D_edit'], self.d_edit_optim
        return self.nets['D'], self.d_optim

    def step(self, g_input, r_input, g_ref, ppl_choice=None, ds_flag=False, extreme_ds_flag=False):
        """One iteration: D, (R1), G, (path length), EMA — the order of train_3_encoder.py:801-822.  Without flags a
        reconstruction iteration.  ds_flag: a dual-supervision batch — D_edit (when given) and its optimiser take D's
        place in the D loss, R1 and the G step's adversarial term (:788-796), and the G step adds the face-regional
        term; extreme_ds_flag: an extreme-pose batch (L1 shrunk, face-id reference = input, face-regional weight 100)."""
        with precision_context(self.args):
            a, n, ld = self.args, self.nets, self.loss_dict
            G, E_Tsr, E_W, E_W_Plus = n['G'], n['E_Tsr'], n['E_W'], n['E_W_Plus']
            Dn, d_optim = self.discriminator(ds_flag)
            D_Loss_BackProp(G, E_Tsr, E_W, E_W_Plus, Dn, g_input, r_input, g_ref, a, ld, d_optim)
            if self.iter_idx % a.d_reg_every == 0:
                ld['r1'] = D_Reg_BackProp(g_ref, Dn, a, d_optim)
            G_Loss_BackProp(G, E_Tsr, E_W, E_W_Plus, Dn, g_input, r_input, g_ref, a, ld, self.g_enc_optim,
                            self.lpips_model, self.face_rec_model, self.fa_model, self.iter_idx, extreme_ds_flag, ds_flag)
            if self.iter_idx % a.g_reg_every == 0 and a.use_g_reg:
                ld['g_reg'], _, self.mean_path_length = G_Reg_BackProp(G, E_Tsr, E_W, E_W_Plus, g_input, r_input, a,
                                                                       self.mean_path_length, self.g_enc_optim, ppl_choice)
            if getattr(a, 'ema_fuse', False) and os.environ.get('FMGAN_NO_EMA_FUSE') != '1':
                self.ema_plan = accumulate_fused(self.g_ema, self.bare['G'], self.accum, self.ema_plan)
            else:
                accumulate(self.g_ema, self.bare['G'], self.accum)
            self.iter_idx += 1
            return ld

    def train_iteration(self, rec_loader, ds_loader, ep_loader=None, ppl_choice=None):
        """One iteration of train()'s schedule (train_3_encoder.py:780-812): the flags, the batch from the loader they
        select (dataset.Data_Loading: reconstruction, partner-paired, or partner-paired extreme pose at half the batch),
        then step().  Loaders are iterators of (photo, render) batches.  Returns (loss_dict, ds_flag, extreme_ds_flag)."""
        ds_flag, extreme_ds_flag = self.ds_flags()
        if extreme_ds_flag and ep_loader is None:
            raise ValueError('train_iteration: an extreme-pose iteration is due (ex_ds_freq) and ep_loader is None')
        device = self.device if self.device is not None else next(self.bare['G'].parameters()).device
        g_input, r_input, g_ref = dataset.Data_Loading(rec_loader, ds_loader, ds_flag, device, extreme_loader=ep_loader,
                                                       extreme_ds_flag=extreme_ds_flag)
        ld = self.step(g_input, r_input, g_ref, ppl_choice, ds_flag, extreme_ds_flag)
        return ld, ds_flag, extreme_ds_flag

    def evaluate(self, rec_eval_loader=None, edit_eval_loader=None, **kwargs):
        """The quantitative half of Sample_Eval_Save_Ckpt (train_3_encoder.py:708-733): Get_Recon_Score on
        rec_eval_loader ((photo, render) batches) and Get_Edit_Score on edit_eval_loader ([photo, render_1, ..] batches),
        with the bare encoders, g_ema, self.face_rec_model and self.lpips_model, under no_grad.  Returns a dict with the
        reference's log names: cos_score, lpips_score, l1_score (reconstruction), cos_score_edit, fid, hmap_score,
        lmark_score, face_reg_score (editing); the scores of a loader that was not given are None, and so are the FID
        and, for a Trainer built without fa_model, hmap_score and lmark_score.  kwargs go to Get_Edit_Score (noise,
        randomize_noise).  Parameters, their requires_grad
        and the modules' training flags, the optimisers, the counters and mean_path_length are left as they are."""
        from Evaluation.quant_eval import Get_Edit_Score, Get_Recon_Score
        a, b = self.args, self.bare
        device = self.device if self.device is not None else next(b['G'].parameters()).device
        generative_model = (b['E_Tsr'], b['E_W'], b['E_W_Plus'], self.g_ema)
        fwd = dict(tsr_encode=a.tsr_encode, sliced_layer=a.w_plus_sliced_layer, use_tanh=a.use_tanh)
        scores = dict.fromkeys(('cos_score', 'lpips_score', 'l1_score', 'cos_score_edit', 'fid', 'hmap_score',
                                'lmark_score', 'face_reg_score'))
        if self.face_rec_model is None or (rec_eval_loader is not None and self.lpips_model is None):
            raise ValueError('evaluate: the Trainer was built without face_rec_model / lpips_model (Module_Fix_Setup)')
        # the reference puts g_ema and the three encoders in eval mode for the evaluation and leaves them there; here every
        # module gets its own flag back
        was_training = [[m.training for m in net.modules()] for net in generative_model]
        try:
            for net in generative_model:
                net.eval()
            with torch.no_grad():
                if rec_eval_loader is not None:
                    scores['cos_score'], scores['lpips_score'], scores['l1_score'] = Get_Recon_Score(
                        rec_eval_loader, device, generative_model, (self.face_rec_model, self.lpips_model), **fwd)
                if edit_eval_loader is not None:
                    (scores['cos_score_edit'], scores['fid'], scores['hmap_score'], scores['lmark_score'],
                     scores['face_reg_score']) = Get_Edit_Score(edit_eval_loader, device, generative_model,
                                                                (self.face_rec_model, None, self.fa_model), **fwd,
                                                                **kwargs)
        finally:
            for net, flags in zip(generative_model, was_training):
                for m, f in zip(net.modules(), flags):
                    m.training = f
        return scores

    # ------------------------------------------------------------------ the rest of Sample_Eval_Save_Ckpt (:667-753)
    def _generative_model(self):
        b = self.bare
        return b['E_Tsr'], b['E_W'], b['E_W_Plus'], self.g_ema

    def sample(self, visual_eval_samples, **sheet_kwargs):
        """The qualitative half (train_3_encoder.py:678-706): Batch_Eval_Sheet of `visual_eval_samples` (the flat list
        of the sample pickers, VAL_SET_LEN images per set) with the bare encoders, g_ema and the args' tsr_encode /
        w_plus_sliced_layer / use_tanh, under no_grad: a uint8 [H, W, 3] tensor on the GPU.  sheet_kwargs: tile, gap,
        margin, background, noise, randomize_noise.  Every module's training flag is restored, as evaluate() does."""
        from Evaluation.visual_eval import Batch_Eval_Sheet
        a = self.args
        generative_model = self._generative_model()
        was_training = [[m.training for m in net.modules()] for net in generative_model]
        try:
            for net in generative_model:
                net.eval()
            with torch.no_grad():
                return Batch_Eval_Sheet(visual_eval_samples, generative_model, tsr_encode=a.tsr_encode,
                                        sliced_layer=a.w_plus_sliced_layer, use_tanh=a.use_tanh, **sheet_kwargs)
        finally:
            for net, flags in zip(generative_model, was_training):
                for m, f in zip(net.modules(), flags):
                    m.training = f

    def checkpoint(self):
        """The reference's checkpoint dict (train_3_encoder.py:737-750: 14 keys, state dicts of the bare modules, None
        for an absent D_edit) plus one key of this build, 'trainer' = {iter_idx, ds_count, mean_path_length}: the three
        counters the reference loses on resume."""
        a, b = self.args, self.bare
        d_edit = b.get('D_edit')
        mpl = self.mean_path_length
        return {
            'g': b['G'].state_dict(),
            'e_tsr': b['E_Tsr'].state_dict(),
            'e_W': b['E_W'].state_dict(),
            'e_W_Plus': b['E_W_Plus'].state_dict(),
            'd': b['D'].state_dict(),
            'd_edit': d_edit.state_dict() if d_edit is not None else None,
            'g_ema': self.g_ema.state_dict(),
            'g_enc_optim': self.g_enc_optim.state_dict(),
            'd_optim': self.d_optim.state_dict(),
            'd_edit_optim': self.d_edit_optim.state_dict() if self.d_edit_optim is not None else None,
            'co_mod': getattr(a, 'co_mod', True),
            'use_tanh': a.use_tanh,
            'tsr_encode': a.tsr_encode,
            'sliced_layer': a.w_plus_sliced_layer,
            'trainer': {'iter_idx': self.iter_idx, 'ds_count': self.ds_count,
                        'mean_path_length': mpl.detach().clone() if torch.is_tensor(mpl) else mpl},
        }

    def save_checkpoint(self, ckpt_dir):
        """Writes ckpt_dir/{iter:06d}.pt for the iteration just finished (self.iter_idx - 1), on rank 0 only; returns
        the path on every rank."""
        import os
        path = os.path.join(ckpt_dir, f'{str(self.iter_idx - 1).zfill(6)}.pt')
        if D_.get_rank() == 0:
            os.makedirs(ckpt_dir, exist_ok=True)
            torch.save(self.checkpoint(), path)
        return path

    def load_checkpoint(self, path_or_dict):
        """Resume from a checkpoint file or dict, this build's or the reference's.  The networks and g_ema are loaded
        through the bare modules, in place, so DDP- or Replica-wrapped networks see the loaded parameters; the
        optimisers through Optimizer_Initilization(..., ckpt=...) over those same parameters.  The counters come from
        'trainer' when present; otherwise by the reference's rule (train_3_encoder.py:438): iter_idx =
        int(path[-9:-3]) + 1, ds_count = 0, mean_path_length = 0.  No derived weight survives a forward here (LiveWeights
        re-reads the parameters at every call), so nothing else needs invalidating."""
        import copy
        b = self.bare
        path = None
        if isinstance(path_or_dict, dict):
            ckpt = path_or_dict
        else:
            path = str(path_or_dict)
            # to the host first: load_state_dict copies into the live tensors wherever they are, and Adam's step counts
            # stay host tensors, as the optimisers keep them
            ckpt = torch.load(path, map_location='cpu', weights_only=False)
        for key, name in (('g', 'G'), ('e_tsr', 'E_Tsr'), ('e_W', 'E_W'), ('e_W_Plus', 'E_W_Plus'), ('d', 'D')):
            b[name].load_state_dict(ckpt[key])
        if b.get('D_edit') is not None and ckpt.get('d_edit') is not None:
            b['D_edit'].load_state_dict(ckpt['d_edit'])
        self.g_ema.load_state_dict(ckpt['g_ema'])
        args = copy.copy(self.args)
        args.load_train_state = True
        self.g_enc_optim, self.d_optim, self.d_edit_optim = Optimizer_Initilization(
            args, b['G'], b['E_Tsr'], b['E_W'], b['E_W_Plus'], b['D'], b.get('D_edit'),
            ckpt=ckpt if ckpt.get('d_edit_optim') is not None else {k: v for k, v in ckpt.items() if k != 'd_edit_optim'})
        state = ckpt.get('trainer')
        if state is not None:
            self.iter_idx, self.ds_count = int(state['iter_idx']), int(state['ds_count'])
            mpl = state['mean_path_length']
            device = self.device if self.device is not None else next(b['G'].parameters()).device
            self.mean_path_length = mpl.detach().to(device, copy=True) if torch.is_tensor(mpl) else mpl
        else:
            if path is None:
                raise ValueError('load_checkpoint: a dict without the \'trainer\' key carries no iteration; pass the '
                                 'file path (the reference reads the iteration from the name, {iter:06d}.pt)')
            self.iter_idx, self.ds_count, self.mean_path_length = int(path[-9:-3]) + 1, 0, 0
        return ckpt

    def Sample_Eval_Save_Ckpt(self, sample_dir, ckpt_dir, visual_eval_samples=None, rec_eval_loader=None,
                              edit_eval_loader=None, log=None):
        """What train() does after every iteration (train_3_encoder.py:667-753), for the iteration just finished, i =
        self.iter_idx - 1: when i % args.val_sample_freq == 0 (and samples were given) the sheet, at tiles of
        args.val_sample_tile, to sample_dir/{i:06d}.png; when i % args.model_save_freq == 0 and i > 0, evaluate() on the given loaders, the
        reference's log text to `log` (a file object), and save_checkpoint(ckpt_dir).  Files are written on rank 0.
        Returns (png path or None, scores or None, checkpoint path or None)."""
        import os
        a = self.args
        i = self.iter_idx - 1
        png = scores = ckpt = None
        if i % a.val_sample_freq == 0 and visual_eval_samples is not None:
            sheet = self.sample(visual_eval_samples, tile=getattr(a, 'val_sample_tile', 256))
            png = os.path.join(sample_dir, f'{str(i).zfill(6)}.png')
            if D_.get_rank() == 0:
                from PIL import Image
                os.makedirs(sample_dir, exist_ok=True)
                Image.fromarray(sheet.cpu().numpy()).save(png)
        if i % a.model_save_freq == 0 and i > 0:
            if rec_eval_loader is not None or edit_eval_loader is not None:
                scores = self.evaluate(rec_eval_loader, edit_eval_loader)
                if log is not None:
                    log.write('\n' + 'Reconstruction Quantitative Evaluation: ' + '\n' +
                              'Cosine Similarity: ' + str(scores['cos_score']) + '\n' +
                              'LPIPS Score: ' + str(scores['lpips_score']) + '\n' +
                              'L1 Score: ' + str(scores['l1_score']) + '\n')
                    log.write('\n' + 'Edit Quantitative Evaluation: ' + '\n' +
                              'Edit Cosine Similarity: ' + str(scores['cos_score_edit']) + '\n' +
                              'FID: ' + str(scores['fid']) + '\n' +
                              'Heat Map: ' + str(scores['hmap_score']) + '\n' +
                              'Land Mark: ' + str(scores['lmark_score']) + '\n' +
                              'Face Regional: ' + str(scores['face_reg_score']) + '\n\n')
            ckpt = self.save_checkpoint(ckpt_dir)
        return png, scores, ckpt


# ====================================================================== the program: arguments, log, train(), main()
def _parse_bool(text):
    """true / false / 1 / 0 (any case).  The reference's type=bool makes every non-empty string True."""
    t = str(text).strip().lower()
    if t in ('true', '1', 'yes'):
        return True
    if t in ('false', '0', 'no'):
        return False
    raise argparse.ArgumentTypeError(f'expected true/false/1/0, got {text!r}')


def _parse_int_list(text):
    """Comma-separated integers ('4,5,6'; 'none' or '' for None).  The reference's type=list splits characters."""
    t = str(text).strip()
    if t.lower() in ('', 'none'):
        return None
    try:
        return [int(v) for v in t.split(',') if v.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f'expected comma-separated integers, got {text!r}') from None


def Args_Parsing(argv=None):
    """The reference's arguments (train_3_encoder.py:52-111), every name, with the defaults default_args() restates from
    train_3_encoder_hyperparams.py.  Differences, on purpose:
      * --synface_dir, --extreme_pose_dir, --ffhq_train_img_dir, --visual_real_img_dir, --quant_eval_img_dir and --ckpt
        default to None (the reference's defaults are its authors' paths); a folder that is None leaves its loaders out;
      * --device defaults to this rank's device (cuda:LOCAL_RANK, or cpu without a GPU), not 'cuda:4';
      * --gpu_device_ids is accepted and ignored: args.n_gpu is the world size of Miscellaneous.distributed (one process
        per GPU) and args.distributed = n_gpu > 1;
      * booleans parse true/false/1/0, --w_plus_sliced_layer and --gpu_device_ids comma-separated integers,
        --hmap_iter_thres a float (so that 'inf', the default, survives).
    This build's own: --log_flush (rows of the loss ledger between two reads of the device, 50), --ema_fuse (the EMA in
    one launch, true), --resident, --bank_cache_dir, --num_workers, --val_sample_tile, --grad_sync (the data path and the
    Trainer's fields of the same names), --exp_dir ('Exp_' + Get_Readable_Cur_Time()), --start_iter (0; a checkpoint
    loaded with --load_train_state sets it), --use_loss_nets (build LPIPS / ArcFace with Module_Fix_Setup, true),
    --precision (fp32 | bf16: Trainer.step under autocast(bfloat16) with the bf16 modulated convolutions; a labelled
    extension, fp32 is the parity path) and --bf16_io (with bf16: 16-bit activations in HBM, precision_context)."""
    d = default_args()
    local = int(os.environ.get('LOCAL_RANK', '0'))
    device = f'cuda:{local % max(torch.cuda.device_count(), 1)}' if torch.cuda.is_available() else 'cpu'
    parser = argparse.ArgumentParser(description='3D-FM GAN, 3-encoder training')
    add = parser.add_argument
    add('--synface_dir', type=str, default=None)
    add('--extreme_pose_dir', type=str, default=None)
    add('--ffhq_train_img_dir', type=str, default=None)
    add('--size', type=int, default=d.size)
    add('--channel_multiplier', type=int, default=2)
    add('--latent', type=int, default=512)
    add('--n_mlp', type=int, default=8)
    add('--use_separate_D', type=_parse_bool, default=True)

    add('--tsr_encode', type=str, default=d.tsr_encode)
    add('--tsr_train', type=_parse_bool, default=d.tsr_train)
    add('--w_encode', type=str, default=MODULATION_ENCODING[0])
    add('--w_train', type=_parse_bool, default=d.w_train)
    add('--w_plus_encode', type=str, default=MODULATION_ENCODING[1])
    add('--w_plus_encoder_layer_num', type=int, default=18)
    add('--w_plus_sliced_layer', type=_parse_int_list, default=d.w_plus_sliced_layer)
    add('--w_plus_train', type=_parse_bool, default=d.w_plus_train)
    add('--co_mod', type=str, default=CO_MODULATION_MODE[0])

    add('--ckpt', type=str, default=None)
    add('--use_tanh', type=_parse_bool, default=d.use_tanh)
    add('--load_train_state', type=_parse_bool, default=True)

    add('--device', type=str, default=device)
    add('--gpu_device_ids', type=_parse_int_list, default=None)

    add('--iter', type=int, default=420001)
    add('--rec_batch', type=int, default=d.rec_batch)
    add('--rec_dataset_type', type=str, default=d.rec_dataset_type)
    add('--ds_batch', type=int, default=d.ds_batch)
    add('--ds_dataset_type', type=str, default=d.ds_dataset_type)
    add('--ds_freq', type=int, default=d.ds_freq)
    add('--ex_ds_freq', type=int, default=d.ex_ds_freq)
    add('--lr', type=float, default=d.lr)

    add('--d_reg_every', type=int, default=d.d_reg_every)
    add('--r1', type=float, default=d.r1)
    add('--use_g_reg', type=_parse_bool, default=d.use_g_reg)
    add('--g_reg_every', type=int, default=d.g_reg_every)
    add('--path_reg_batch_shrink', type=int, default=d.path_reg_batch_shrink)
    add('--generator_path_reg_weight', type=float, default=d.generator_path_reg_weight)

    add('--l1_loss_lambda', type=float, default=d.l1_loss_lambda)
    add('--lpips_loss_lambda', type=float, default=d.lpips_loss_lambda)
    add('--ep_lpips_l1_weight_shrink', type=float, default=d.ep_lpips_l1_weight_shrink)
    add('--face_id_loss_lambda', type=float, default=d.face_id_loss_lambda)
    add('--face_id_loss_type', type=str, default=d.face_id_loss_type)
    add('--hmap_loss_lambda', type=float, default=d.hmap_loss_lambda)
    add('--hmap_iter_thres', type=float, default=d.hmap_iter_thres)
    add('--rec_face_reg_loss_lambda', type=float, default=d.rec_face_reg_loss_lambda)
    add('--ds_face_reg_loss_lambda', type=float, default=d.ds_face_reg_loss_lambda)
    add('--ep_face_reg_loss_lambda', type=float, default=d.ep_face_reg_loss_lambda)

    add('--n_real_eval_faces', type=int, default=d.n_real_eval_faces)
    add('--n_syn_eval_faces', type=int, default=d.n_syn_eval_faces)
    add('--visual_real_img_dir', type=str, default=None)
    add('--val_sample_freq', type=int, default=d.val_sample_freq)
    add('--model_save_freq', type=int, default=d.model_save_freq)
    add('--quant_eval_img_dir', type=str, default=None)
    add('--quant_eval_batch_size', type=int, default=d.quant_eval_batch_size)

    add('--log_flush', type=int, default=50)
    add('--ema_fuse', type=_parse_bool, default=True)
    add('--resident', type=_parse_bool, default=True)
    add('--bank_cache_dir', type=str, default=d.bank_cache_dir)
    add('--num_workers', type=int, default=d.num_workers)
    add('--val_sample_tile', type=int, default=d.val_sample_tile)
    add('--grad_sync', type=str, default=d.grad_sync, choices=('ddp', 'flat'))
    add('--exp_dir', type=str, default=None)
    add('--start_iter', type=int, default=0)
    add('--use_loss_nets', type=_parse_bool, default=True)
    add('--precision', type=str, default='fp32', choices=('fp32', 'bf16'))
    add('--bf16_io', type=_parse_bool, default=BF16_IO_DEFAULT)

    args = parser.parse_args(argv)
    if args.exp_dir is None:
        args.exp_dir = 'Exp_' + Get_Readable_Cur_Time()
    args.n_gpu = D_.get_world_size()
    args.distributed = args.n_gpu > 1
    return args


def Get_Readable_Cur_Time():
    import datetime
    return datetime.datetime.now().strftime("%Y-%m-%d_%H:%M:%S")


# (label, field of args) of Print_Experiment_Status, section by section (train_3_encoder.py:124-184)
_STATUS_SECTIONS = (
    ('  Model and Training Data: ', (
        ('Synthetic Data Folder', 'synface_dir'), ('Extreme Pose Data Folder', 'extreme_pose_dir'),
        ('FFHQ Data Folder', 'ffhq_train_img_dir'), ('Generator Num Layers', 'n_latent'),
        ('Latent Variable Dimension', 'latent'), ('Generated Image Size', 'size'),
        ('Channel Multiplier', 'channel_multiplier'), ('Using Separate Discriminator', 'use_separate_D'),
        ('Tensor Encoding', 'tsr_encode'), ('E_Tsr Trainable', 'tsr_train'), ('W Space Encoding', 'w_encode'),
        ('E_W Trainable', 'w_train'), ('W+ Space Encoding', 'w_plus_encode'),
        ('W+ Space Layer Slicing', 'w_plus_sliced_layer'), ('E_W+ Trainable', 'w_plus_train'),
        ('Num W+ Encoder Layer', 'w_plus_encoder_layer_num'), ('Co-Modulation', 'co_mod'), ('Tanh Clipping', 'use_tanh'),
        ('Initial Checkpoint', 'ckpt'), ('Load Training State', 'load_train_state'))),
    ('  GPU Setup: ', (
        ('Distributed Training', 'distributed'), ('Primiary GPU Device', 'device'), ('GPU Device IDs', 'gpu_device_ids'),
        ('Number of GPUs', 'n_gpu'))),
    ('  Training Params: ', (
        ('Training Iterations', 'iter'), ('Reconstruction Dataset', 'rec_dataset_type'),
        ('Reconstruction Batch Size', 'rec_batch'), ('Dual Supervision Dataset', 'ds_dataset_type'),
        ('Dual Supervision Batch Size', 'ds_batch'), ('Dual Supervision Frequency', 'ds_freq'),
        ('Extreme Disentangled Supervision Frequency', 'ex_ds_freq'), ('Learning Rate', 'lr'),
        ('Use Generator Regularization', 'use_g_reg'), ('Generator Regularization Frequency', 'g_reg_every'),
        ('Generator Regularization Weight', 'generator_path_reg_weight'),
        ('Generator Regularization Batch Shrink', 'path_reg_batch_shrink'),
        ('Discriminator Regularization Frequency', 'd_reg_every'), ('Discriminator Regularization Weight', 'r1'),
        ('LPIPS Loss Weight', 'lpips_loss_lambda'), ('L1 Loss Weight', 'l1_loss_lambda'),
        ('L1 LPIPS Weight Shrink for Extreme Pose', 'ep_lpips_l1_weight_shrink'),
        ('Face ID Loss Weight', 'face_id_loss_lambda'), ('Face ID Loss Type', 'face_id_loss_type'),
        ('Heat Map Loss Weight', 'hmap_loss_lambda'), ('Heat Map Loss Iteration Threshold', 'hmap_iter_thres'),
        ('Reconstruction Face Regional Loss Weight', 'rec_face_reg_loss_lambda'),
        ('Disentanglement Face Regional Loss Weight', 'ds_face_reg_loss_lambda'),
        ('Extreme Pose Face Regional Loss Weight', 'ep_face_reg_loss_lambda'))),
    ('  Validation Params: ', (
        ('Model Saving Frequency', 'model_save_freq'), ('Quantitative Evaluation Directory', 'quant_eval_img_dir'),
        ('Quantitative Evaluation Batch Size', 'quant_eval_batch_size'), ('Visual Evaluation Frequency', 'val_sample_freq'),
        ('Number of Visual Real Samples', 'n_real_eval_faces'), ('Number of Visual Synthetic Samples', 'n_syn_eval_faces'),
        ('Visual Real Samples Directory', 'visual_real_img_dir'))),
)


def Experiment_Status_Text(args):
    """The text Print_Experiment_Status prints and writes: the reference's, character for character (:124-184)."""
    text = '\n' + '--------------- Training Start ---------------' + '\n\n' + 'Params: ' + '\n\n'
    for title, fields in _STATUS_SECTIONS:
        text += title + '\n'
        text += '\n'.join('    ' + label + ': ' + str(getattr(args, field)) for label, field in fields) + '\n\n'
    return text


def Precision_Status_Text(args):
    """This build's own line after the reference's text: the precision Trainer.step runs in.  Settings without the field
    (default_args(), the reference's own) are fp32 and print the reference's text alone."""
    if not hasattr(args, 'precision'):
        return ''
    precision = args.precision
    text = '  Precision: ' + str(precision)
    if precision == 'bf16':
        on = training_precision(args)[1]
        text += ' (16-bit activation kernels: ' + ('on' if on else 'off') + ')'
    return text + '\n\n'


def Print_Experiment_Status(args, exp_log_file):
    """Prints the experiment's settings and writes them to the log (train_3_encoder.py:119-187), then the precision line;
    rank 0 only."""
    if D_.get_rank() != 0:
        return
    text = Experiment_Status_Text(args) + Precision_Status_Text(args)
    print(text)
    if exp_log_file is not None:
        exp_log_file.write(text)


def Module_To_Train_Setup(args):
    """The networks to train (train_3_encoder.py:311-364): (G, E_Tsr, E_W, E_W_Plus, D, D_edit, g_ema, ckpt), bare
    modules on args.device — Trainer wraps them for data parallelism, there is no nn.DataParallel.  D_edit exists under
    the reference's condition (:325); with args.ckpt the reference's loading rules (:332-345); without one g_ema starts
    as a copy of G (accumulate(g_ema, G, 0)).  The Generators of a checkpoint are built with args.n_mlp (the reference
    leaves Build_Generator_From_Dict's default of 8 there, which is its own --n_mlp default).  Sets args.n_latent."""
    import math
    import resnet_encoder
    from psp_encoder_model.encoders import psp_encoders
    from stylegan2 import Discriminator, Generator
    from Util.network_util import Build_Generator_From_Dict
    device = args.device
    E_Tsr = resnet_encoder.resnet18(tensor_encoding=True).to(device)
    E_W = resnet_encoder.resnet18(tensor_encoding=False).to(device)
    opts = types.SimpleNamespace(input_nc=3, n_styles=int(math.log(args.size, 2)) * 2 - 2)
    E_W_Plus = psp_encoders.GradualStyleEncoder(args.w_plus_encoder_layer_num, 'ir_se', opts).to(device)
    D = Discriminator(args.size, channel_multiplier=args.channel_multiplier).to(device)
    D_edit = None
    if args.rec_dataset_type == 'FFHQ' and args.ds_dataset_type == 'Synthetic' and args.use_separate_D:
        D_edit = Discriminator(args.size, channel_multiplier=args.channel_multiplier).to(device)
    ckpt = None
    if args.ckpt is not None:
        ckpt = torch.load(args.ckpt, map_location='cpu', weights_only=False)
        G = Build_Generator_From_Dict(ckpt['g'], size=args.size, latent=args.latent, n_mlp=args.n_mlp).to(device)
        g_ema = Build_Generator_From_Dict(ckpt['g_ema'], size=args.size, latent=args.latent, n_mlp=args.n_mlp).to(device)
        D.load_state_dict(ckpt['d'])
        if 'e_tsr' in ckpt and 'e_W' in ckpt and 'e_W_Plus' in ckpt:
            E_Tsr.load_state_dict(ckpt['e_tsr'], strict=False)
            E_W.load_state_dict(ckpt['e_W'], strict=False)
            E_W_Plus.load_state_dict(ckpt['e_W_Plus'], strict=False)
        if D_edit is not None:
            D_edit.load_state_dict(ckpt['d_edit'] if ckpt.get('d_edit') is not None else ckpt['d'])
    else:
        G = Generator(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier).to(device)
        g_ema = Generator(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier).to(device)
        accumulate(g_ema, G, 0)
    g_ema.eval()
    args.n_latent = g_ema.n_latent
    return G, E_Tsr, E_W, E_W_Plus, D, D_edit, g_ema, ckpt


def Training_Setup(exp_dir, args):
    """(sample_dir, ckpt_dir) below exp_dir (train_3_encoder.py:604-607), created on rank 0."""
    sample_dir = os.path.join(exp_dir, 'sample') + '/'
    ckpt_dir = os.path.join(exp_dir, 'ckpt') + '/'
    if D_.get_rank() == 0:
        os.makedirs(sample_dir, exist_ok=True)
        os.makedirs(ckpt_dir, exist_ok=True)
    return sample_dir, ckpt_dir


def Train_Status_Line(iter_idx, seconds, ds_flag, extreme_ds_flag, values):
    """The reference's log line of one iteration (train_3_encoder.py:655) from a dict of Python floats keyed by the
    ledger's names; a name that is missing counts as 0.0."""
    v = lambda name: str(round(float(values.get(name, 0.0)), 3))        # noqa: E731
    return ('Iter #: ' + str(iter_idx) + ' Train Time: ' + str(round(seconds, 2)) + ' Dual Supervision: ' + str(ds_flag) +
            ' Extreme Pose DS: ' + str(extreme_ds_flag) + ' D_Loss: ' + v('d') + ' G_Loss: ' + v('g') + ' G_Reg: ' +
            v('g_reg') + ' L1_Loss: ' + v('l1') + ' LPIPS_Loss: ' + v('lpips') + ' Face_ID_Loss: ' + v('face_id') +
            ' Heat_Map_Loss: ' + v('hmap') + ' Face_Regional_Loss: ' + v('face_reg') + '\n')


def Print_Train_Status(rows, exp_log_file):
    """One line per row of LossLedger.flush() into the log, on rank 0 (the other ranks' flush returns no rows)."""
    if exp_log_file is None or D_.get_rank() != 0:
        return
    for iter_idx, seconds, ds_flag, extreme_ds_flag, values in rows:
        exp_log_file.write(Train_Status_Line(iter_idx, seconds, ds_flag, extreme_ds_flag, values))


def train(args, train_loaders, eval_loaders, trainer, visual_eval_samples, exp_dir, exp_log_file, ledger=None):
    """The loop of train_3_encoder.py:756-828 over a Trainer: train_loaders = (rec, ds, ep, pure FFHQ) streams and
    eval_loaders = (rec_eval, edit_eval), as Dataset_DataLoader_Setup returns them.  The trainer is touched only through
    iter_idx, train_iteration and Sample_Eval_Save_Ckpt.

    The loss values go through an op.loss_log.LossLedger of args.log_flush rows (returned; `ledger`: one to use
    instead): an iteration adds one launch and two event records, and the log lines are written when the ring is full,
    before an evaluation block (so that the file keeps the reference's order) and, in `finally`, at the end — an
    exception leaves the line of every finished iteration in the file.  Between flushes the loop synchronises nothing
    and copies nothing to the host.  The time in a line is the device time between the iteration's first and last
    launch (events), where the reference prints the host clock over the same span."""
    from op.loss_log import LossLedger
    rec_train_loader, ds_train_loader, ep_train_loader = train_loaders[:3]
    rec_eval_loader, edit_eval_loader = eval_loaders
    sample_dir, ckpt_dir = Training_Setup(exp_dir, args)
    if ledger is None:
        device = getattr(trainer, 'device', None)
        device = device if device is not None else getattr(args, 'device', 'cpu')
        ledger = LossLedger(device, max(1, int(getattr(args, 'log_flush', 50))))

    def flush():
        Print_Train_Status(ledger.flush(), exp_log_file)

    try:
        while trainer.iter_idx < args.iter:
            iter_idx = trainer.iter_idx
            ledger.begin()
            loss_dict, ds_flag, extreme_ds_flag = trainer.train_iteration(rec_train_loader, ds_train_loader, ep_train_loader)
            ledger.write(iter_idx, loss_dict, ds_flag, extreme_ds_flag)
            # Sample_Eval_Save_Ckpt's own condition for the evaluation text and the checkpoint (:708)
            evaluates = iter_idx % args.model_save_freq == 0 and iter_idx > 0
            if ledger.full() or evaluates:
                flush()
            trainer.Sample_Eval_Save_Ckpt(sample_dir, ckpt_dir, visual_eval_samples, rec_eval_loader, edit_eval_loader,
                                          log=exp_log_file)
    finally:
        flush()
    return ledger


def main(argv=None):
    """train_3_encoder.py:831-875 on one process per GPU: the arguments, the data, the networks, the frozen loss networks,
    the Trainer (resumed from --ckpt when --load_train_state), the experiment folder and its log, the loop."""
    import time
    rank, world, device = D_.init_distributed()
    args = Args_Parsing(argv)
    device = torch.device(args.device)
    (transform, synface_dataset, extreme_pose_dataset, rec_train_loader, ds_train_loader, ep_train_loader,
     pure_ffhq_loader, rec_eval_loader, edit_eval_loader) = Dataset_DataLoader_Setup(args, device, resident=args.resident)
    G, E_Tsr, E_W, E_W_Plus, D, D_edit, g_ema, ckpt = Module_To_Train_Setup(args)
    lpips_model = face_rec_model = None
    if args.use_loss_nets:
        lpips_model, face_rec_model = Module_Fix_Setup(args, device)
    nets = dict(G=G, E_Tsr=E_Tsr, E_W=E_W, E_W_Plus=E_W_Plus, D=D)
    if D_edit is not None:
        nets['D_edit'] = D_edit
    trainer = Trainer(nets, args, device, g_ema=g_ema, lpips_model=lpips_model, face_rec_model=face_rec_model)
    trainer.iter_idx = args.start_iter
    if args.ckpt is not None and args.load_train_state:
        trainer.load_checkpoint(args.ckpt)
        args.start_iter = trainer.iter_idx

    exp_dir = args.exp_dir
    exp_log_file = None
    if rank == 0:
        os.makedirs(exp_dir, exist_ok=True)
        exp_log_file = open(os.path.join(exp_dir, Get_Readable_Cur_Time() + '_training_log.out'), 'w')
    D_.synchronize()
    try:
        Print_Experiment_Status(args, exp_log_file)
        visual_eval_samples = None
        if args.visual_real_img_dir is not None and synface_dataset is not None and extreme_pose_dataset is not None:
            visual_eval_samples = Visual_Evaluation_Setup(args, synface_dataset, extreme_pose_dataset, transform, device)
        train_start_time = time.time()
        train_loaders = rec_train_loader, ds_train_loader, ep_train_loader, pure_ffhq_loader
        eval_loaders = rec_eval_loader, edit_eval_loader
        train(args, train_loaders, eval_loaders, trainer, visual_eval_samples, exp_dir, exp_log_file)
        if device.type == 'cuda':
            torch.cuda.synchronize(device)
        train_end_time = time.time()
        if exp_log_file is not None:
            exp_log_file.write('\n' + 'Total training time: ' + str(round(train_end_time - train_start_time, 3)))
    finally:
        if exp_log_file is not None:
            exp_log_file.close()
    return exp_dir


if __name__ == '__main__':
    main()
