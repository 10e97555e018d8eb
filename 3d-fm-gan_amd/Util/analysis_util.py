"""Reading a training log back (Util/analysis_util.py of the reference): the loss values of the iteration lines
train_3_encoder.Train_Status_Line writes, the scores of the two evaluation blocks Trainer.Sample_Eval_Save_Ckpt writes,
and the inference models of a checkpoint (both schemes).  The parsing functions return what the reference's return on
the same text.  Not provided: the loss-curve figure (no matplotlib, no easydict here)."""
import math
import types


def Parse_A_Line(log_line):
    """(D_Loss, G_Loss) of one iteration line (:24-37).  The reference reads G_Loss up to 'L1_Loss: ', which is right for
    the lines of its 2-encoder script; on a line of train_3_encoder.py, where ' G_Reg: ' stands in between, its float()
    raises ValueError.  Here the G_Loss field ends at 'G_Reg: ' when that comes first: the reference's result wherever
    it has one, and the two values on the lines this build writes."""
    d_loss_str, g_loss_str, g_reg_str, l1_loss_str = 'D_Loss: ', 'G_Loss: ', 'G_Reg: ', 'L1_Loss: '
    d_loss_start = log_line.find(d_loss_str) + len(d_loss_str)
    d_loss_end = log_line.find(g_loss_str)
    d_loss = float(log_line[d_loss_start:d_loss_end])
    g_loss_start = log_line.find(g_loss_str) + len(g_loss_str)
    g_loss_end = log_line.find(l1_loss_str)
    g_reg_at = log_line.find(g_reg_str, g_loss_start)
    if g_reg_at != -1 and (g_loss_end == -1 or g_reg_at < g_loss_end):
        g_loss_end = g_reg_at
    g_loss = float(log_line[g_loss_start:g_loss_end])
    return d_loss, g_loss


def Moving_Average(list_or_array):
    """The running mean of a list or array, as a list (:39-56)."""
    running_mean = [list_or_array[0]]
    for i in range(1, len(list_or_array)):
        new_sample_weight = 1 / (i + 1)
        running_mean.append(running_mean[i - 1] * (1 - new_sample_weight) + list_or_array[i] * new_sample_weight)
    assert len(running_mean) == len(list_or_array)
    return running_mean


def Extract_Reconstruction_Evaluation_Score(exp_log_file):
    """(cosine similarity, LPIPS, L1) lists of the reconstruction blocks of a log file (:59-88)."""
    cos_str, lpips_str, l1_str = 'Cosine Similarity: ', 'LPIPS Score: ', 'L1 Score: '
    cos_list, lpips_list, l1_list = [], [], []
    with open(exp_log_file, 'r') as f:
        for line in f.readlines():
            if (cos_str in line) and ('Edit' not in line):
                cos_list.append(float(line[len(cos_str):]))
            elif lpips_str in line:
                lpips_list.append(float(line[len(lpips_str):]))
            elif l1_str in line:
                l1_list.append(float(line[len(l1_str):]))
    return cos_list, lpips_list, l1_list


def Extract_Edit_Evaluation_Score(exp_log_file):
    """(edit cosine similarity, FID, heat map, land mark, face regional) lists of the editing blocks (:91-132)."""
    cos_str, fid_str, hmap_str, lmark_str, face_reg_str = ('Edit Cosine Similarity: ', 'FID: ', 'Heat Map: ', 'Land Mark: ',
                                                           'Face Regional:')
    cos_list, fid_list, hmap_list, lmark_list, face_reg_list = [], [], [], [], []
    with open(exp_log_file, 'r') as f:
        for line in f.readlines():
            if cos_str in line:
                cos_list.append(float(line[len(cos_str):]))
            elif fid_str in line:
                fid_list.append(float(line[len(fid_str):]))
            elif hmap_str in line:
                hmap_list.append(float(line[len(hmap_str):]))
            elif lmark_str in line:
                lmark_list.append(float(line[len(lmark_str):]))
            elif face_reg_str in line:
                face_reg_list.append(float(line[len(face_reg_str):]))
    return cos_list, fid_list, hmap_list, lmark_list, face_reg_list


def Model_Building_Func_3_Encoder(ckpt_model, device, gpu_device_ids=None):
    """(g_ema, E_Tsr, E_W, E_W_Plus) of a checkpoint dict as bare eval-mode modules on `device` (:204-243): size 256,
    latent 512, the pSp depth from the number of keys of ckpt_model['e_W_Plus'] (325 -> 18).  565 keys mean the 50-layer
    body, which this build does not provide: ValueError, as for any other count (where the reference fails with an
    unbound name).  gpu_device_ids is ignored: there is no nn.DataParallel."""
    import resnet_encoder
    from psp_encoder_model.encoders import psp_encoders
    from .network_util import Build_Generator_From_Dict
    n_keys = len(ckpt_model['e_W_Plus'].keys())
    if n_keys != 325:
        raise ValueError(f'Model_Building_Func_3_Encoder: e_W_Plus has {n_keys} keys; 325 (the 18-layer pSp body) is the '
                         f'one provided' + (' (565: the 50-layer body is not)' if n_keys == 565 else ''))
    wplus_mod_layer, size, latent_dim = 18, 256, 512
    g_ema = Build_Generator_From_Dict(ckpt_model['g_ema'], size=size, latent=latent_dim).to(device)
    E_Tsr = resnet_encoder.resnet18(tensor_encoding=True).to(device)
    E_W = resnet_encoder.resnet18(tensor_encoding=False).to(device)
    opts = types.SimpleNamespace(input_nc=3, n_styles=int(math.log(size, 2)) * 2 - 2)
    E_W_Plus = psp_encoders.GradualStyleEncoder(wplus_mod_layer, 'ir_se', opts).to(device)
    E_Tsr.load_state_dict(ckpt_model['e_tsr'])
    E_W.load_state_dict(ckpt_model['e_W'])
    E_W_Plus.load_state_dict(ckpt_model['e_W_Plus'])
    return g_ema.eval(), E_Tsr.eval(), E_W.eval(), E_W_Plus.eval()


def _psp_depth(e_w_dict):
    """Depth of the pSp body a state dict was saved from, read off its number of units (`body.N.`): 8 units are the
    18-layer body (the reference's 325-key dict at 14 styles), 24 the 50-layer one (565 keys) — whatever the number of
    style heads.  Anything else: ValueError naming the key count (the reference leaves its variable unbound there)."""
    units = {k.split('.')[1] for k in e_w_dict.keys() if k.startswith('body.')}
    depth = {8: 18, 24: 50}.get(len(units))
    if depth is None:
        raise ValueError(f'Model_Building_Func_2_Encoder: e_W has {len(e_w_dict.keys())} keys and {len(units)} body units; '
                         f'8 units (the 18-layer pSp body, 325 keys) or 24 (the 50-layer one, 565 keys) are recognised')
    return depth


def Model_Building_Func_2_Encoder(ckpt_model, device, gpu_device_ids=None):
    """(g_ema, E_Tsr, E_W, mod_encode, co_mod) of a checkpoint dict of the 2-encoder scheme (:135-201), the modules bare
    and in eval mode on `device` as Model_Building_Func_3_Encoder builds its own.  Defaults where the checkpoint has no
    mode keys: mod_space 'W', mod_encode 'Render Image', co_mod None; co_mod True means 'Multiplication'.  Size 256; the
    Generator's style_dim is 1024 for 'Concatenation' and 'Tensor Transform', else 512.  The tensor encoder is
    resnet18(tensor_encoding=True) in the plain mode, with tensor_transform=True for 'Tensor Transform', and the vector
    form (tensor_encoding=False) for the other two co-modulation modes; the modulation encoder is the vector ResNet for
    mod_space 'W' in the plain mode and the pSp encoder otherwise, with the 14 styles of size 256 and its depth read
    off ckpt_model['e_W'].  gpu_device_ids is ignored: there is no nn.DataParallel."""
    import resnet_encoder
    from psp_encoder_model.encoders import psp_encoders
    from .network_util import CO_MODULATION_MODE, MODULATION_ENCODING, Build_Generator_From_Dict
    mod_space = ckpt_model['mod_space'] if 'mod_space' in ckpt_model.keys() else 'W'
    mod_encode = ckpt_model['mod_encode'] if 'mod_encode' in ckpt_model.keys() else 'Render Image'
    co_mod = ckpt_model['co_mod'] if 'co_mod' in ckpt_model.keys() else None
    if co_mod is True:
        co_mod = 'Multiplication'
    elif co_mod is False:
        co_mod = None
    if mod_space not in ('W', 'W+') or mod_encode not in MODULATION_ENCODING or (
            co_mod is not None and co_mod not in CO_MODULATION_MODE):
        raise ValueError(f'Model_Building_Func_2_Encoder: mod_space {mod_space!r}, mod_encode {mod_encode!r}, '
                         f'co_mod {co_mod!r} is not a mode of the 2-encoder scheme')
    size = 256
    latent_dim = 1024 if co_mod in ('Concatenation', 'Tensor Transform') else 512
    g_ema = Build_Generator_From_Dict(ckpt_model['g_ema'], size=size, latent=latent_dim).to(device)
    if co_mod is None:
        E_Tsr = resnet_encoder.resnet18(tensor_encoding=True)
    elif co_mod == 'Tensor Transform':
        E_Tsr = resnet_encoder.resnet18(tensor_encoding=True, tensor_transform=True)
    else:
        E_Tsr = resnet_encoder.resnet18(tensor_encoding=False)
    if co_mod is None and mod_space == 'W':
        E_W = resnet_encoder.resnet18(tensor_encoding=False)
    else:
        opts = types.SimpleNamespace(input_nc=3, n_styles=int(math.log(size, 2)) * 2 - 2)
        E_W = psp_encoders.GradualStyleEncoder(_psp_depth(ckpt_model['e_W']), 'ir_se', opts)
    E_Tsr, E_W = E_Tsr.to(device), E_W.to(device)
    E_Tsr.load_state_dict(ckpt_model['e_tsr'])
    E_W.load_state_dict(ckpt_model['e_W'])
    return g_ema.eval(), E_Tsr.eval(), E_W.eval(), mod_encode, co_mod
