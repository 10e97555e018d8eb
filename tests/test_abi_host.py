"""CPU tests of the boundary and the host logic: the C-ABI library loads and exports every symbol the header
declares, pure-host entry points behave, the product has NO CPU path, and the product modules keep the
reference's parameter/buffer names and shapes (manifests captured from the reference)."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import cases
import synth
from nets import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_header_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'fmgan_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    names = sorted(set(re.findall(r'\b(fmgan_\w+)\s*\(', hdr)))
    assert len(names) >= 11
    L = lib()
    for n in names:
        assert hasattr(L, n), f'{n} declared in include/fmgan_hip.h but not exported'
    assert L.fmgan_abi_version() == 1
    assert L.fmgan_status_string(0) == b'ok'
    assert b'invalid' in L.fmgan_status_string(-1)


def test_signature_table_matches_header():
    """The argtypes / restype table of _native.lib() against include/fmgan_hip.h, declaration by declaration: a miscounted
    int / long long / float in the table would hand a kernel garbage pointers.  The rule: every pointer parameter is bound
    as c_void_p (the wrappers pass data_ptr() integers or None), except `int *`: the host-side out-parameters the wrappers
    fill through ctypes.byref or a ctypes array (fmgan_upfirdn2d_out_size, fmgan_modconv2d_select, ...) are
    POINTER(c_int), and only an `int *` named `plan` — the resize table, handed over as the raw address of an int32
    tensor, host or device — is c_void_p.  `const char *` is returned as c_char_p; int, long long and float map to c_int,
    c_longlong and c_float."""
    hdr = open(os.path.join(ROOT, 'include', 'fmgan_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    hdr = re.sub(r'^\s*#.*$', '', hdr, flags=re.M)
    scalars = {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'float': ctypes.c_float}

    def ctype_of(decl, is_return=False):
        """ctypes forms the table may use for a C type; `decl` still carries the parameter name unless is_return."""
        decl = ' '.join(decl.replace('*', ' * ').split())
        if '*' in decl:
            base = decl[:decl.index('*')].replace('const', '').strip()
            if is_return:
                assert base == 'char', decl
                return (ctypes.c_char_p,)
            by_ref = base == 'int' and not decl.endswith('* plan')
            return (ctypes.POINTER(ctypes.c_int),) if by_ref else (ctypes.c_void_p,)
        words = decl.split() if is_return else decl.split()[:-1]
        return (scalars[' '.join(words)],)

    decls = re.findall(r'([\w \t*]+?)\b(fmgan_\w+)\s*\(([^()]*)\)\s*;', hdr)
    assert len(decls) == len(re.findall(r'\bfmgan_\w+\s*\(', hdr)) == len({name for _, name, _ in decls})
    L = lib()
    for ret, name, params in decls:
        fn = getattr(L, name)
        assert fn.argtypes is not None, f'{name} is declared in the header but lib() gives it no signature'
        want = [] if params.strip() == 'void' else [ctype_of(p) for p in params.split(',')]
        assert len(fn.argtypes) == len(want), f'{name}: {len(fn.argtypes)} argtypes for {len(want)} parameters'
        for k, (got, ok) in enumerate(zip(fn.argtypes, want)):
            assert got in ok, f'{name} parameter {k}: bound as {got.__name__}, the header wants {[t.__name__ for t in ok]}'
        assert fn.restype in ctype_of(ret, is_return=True), f'{name}: restype {fn.restype}'
    bound = [n for n, fn in vars(L).items() if n.startswith('fmgan_') and fn.argtypes is not None]
    assert len(bound) == len(decls), set(bound) ^ {name for _, name, _ in decls}


def test_out_size_matches_reference_formula():
    from op import _native
    for c in cases.UPFIRDN2D_CASES:
        k = cases.make_fir(c['kernel'])
        h, w = c['shape'][2:]
        p0, p1 = c['pad']
        oh, ow = _native.upfirdn2d_out_size(h, w, k.shape[0], k.shape[1], c['up'], c['up'], c['down'], c['down'],
                                           p0, p1, p0, p1)
        # op/upfirdn2d.py:112-113
        assert oh == (h * c['up'] + p0 + p1 - k.shape[0]) // c['down'] + 1
        assert ow == (w * c['up'] + p0 + p1 - k.shape[1]) // c['down'] + 1


def test_path_selection_is_host_logic():
    L = lib()
    # headline blur [256,1025,1025] -> row-march; 9x9 plane -> not row-march; f64 -> generic; bad args -> EINVAL
    assert L.fmgan_upfirdn2d_select(0, 256, 1025, 1025, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == 1
    assert L.fmgan_upfirdn2d_select(0, 1024, 9, 9, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) != 1
    assert L.fmgan_upfirdn2d_select(1, 256, 1025, 1025, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == 0
    assert L.fmgan_upfirdn2d_select(0, 1, 0, 8, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == -1
    assert L.fmgan_upfirdn2d_select(7, 1, 8, 8, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == -2


def test_invalid_arguments_return_status_without_gpu():
    L = lib()
    # null pointers / bad dims are rejected before any HIP call
    assert L.fmgan_upfirdn2d(0, None, None, None, 1, 8, 8, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, -1, None) == -1
    assert L.fmgan_upfirdn2d(0, None, None, None, 1, 8, 8, 1, 4, 4, 0, 1, 1, 1, 1, 1, 1, 1, -1, None) == -1
    assert L.fmgan_fused_bias_act(0, None, None, None, None, 16, 0, 1, 3, 0, 0.2, 1.4, None) == -1
    assert L.fmgan_fused_bias_act(9, None, None, None, None, 16, 0, 1, 3, 0, 0.2, 1.4, None) == -2
    assert L.fmgan_modconv2d_f32(None, None, None, None, None, 1, 8, 8, 4, 4, 3, None, None, None, 1, 0, 0.2, 1.4, 0, 0, None, 0, None) == -2
    assert L.fmgan_modconv2d_f32(None, None, None, None, None, 1, 8, 8, 4, 4, 0, None, None, None, 1, 0, 0.2, 1.4, 0, 0, None, 0, None) == -1
    assert L.fmgan_torgb_f32(None, None, None, None, None, None, 1, 8, 5, 16, 1.0, None) == -1
    # split-K workspace query is pure host logic: tiny layer -> non-zero, big layer -> 0
    assert L.fmgan_modconv2d_workspace_bytes(8, 512, 512, 4, 4, 0) > 0
    assert L.fmgan_modconv2d_workspace_bytes(8, 32, 32, 1024, 1024, 0) == 0
    # empty batch is a no-op
    assert L.fmgan_upfirdn2d(0, None, None, None, 0, 8, 8, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, -1, None) == 0


def test_prelu_backward_host_logic():
    """fmgan_prelu_backward_blocks / _f32: partial-sum rows per launch and argument checks, all before any HIP call."""
    L = lib()
    assert L.fmgan_prelu_backward_blocks(0, 64) == 0 and L.fmgan_prelu_backward_blocks(10, 0) == 0
    for rows, c in ((1, 64), (1 << 20, 64), (1 << 20, 512), (300, 96), (7, 2048)):
        b = L.fmgan_prelu_backward_blocks(rows, c)
        q = 1
        while q < c // 4 and q < 256:
            q *= 2
        assert 1 <= b <= max(1, -(-rows // (256 // q))) and b <= 256 * 8        # never more blocks than row groups / 8 per CU
    assert L.fmgan_prelu_backward_f32(None, None, None, None, None, 0, 64, None) == 0          # empty: nothing to do
    assert L.fmgan_prelu_backward_f32(None, None, None, None, None, 16, 64, None) == -1        # null pointers
    assert L.fmgan_prelu_backward_f32(None, None, None, None, None, 16, 6, None) == -2         # channels % 4: unsupported
    assert L.fmgan_prelu_backward_f32(None, None, None, None, None, -1, 64, None) == -1


def test_fused_bias_act_backward_host_logic():
    """fmgan_fused_bias_act_bwd_blocks / _f32: which planes the one-pass backward serves, partial columns per plane,
    argument checks — all before any HIP call."""
    L = lib()
    for planes, hw, want in ((0, 64, 0), (8, 16, 0), (8, 63, 0), (8, 66, 0), (8, 64, 1), (8, 4096, 1), (8, 4100, 2),
                             (256, 1024 * 1024, 64), (1 << 31, 64, 0)):
        assert L.fmgan_fused_bias_act_bwd_blocks(planes, hw) == want, (planes, hw)
    assert L.fmgan_fused_bias_act_bwd_f32(None, None, None, None, 0, 64, 0.2, 1.4, None) == 0       # empty
    assert L.fmgan_fused_bias_act_bwd_f32(None, None, None, None, 4, 64, 0.2, 1.4, None) == -1      # null pointers
    assert L.fmgan_fused_bias_act_bwd_f32(None, None, None, None, -1, 64, 0.2, 1.4, None) == -1
    assert L.fmgan_fused_bias_act_bwd_f32(16, 16, 16, 16, 4, 30, 0.2, 1.4, None) == -2              # unserved plane size
    assert L.fmgan_fused_bias_act_bwd_f32(20, 16, 16, 16, 4, 64, 0.2, 1.4, None) == -2              # misaligned


def test_torgb_backward_host_logic():
    L = lib()
    assert L.fmgan_torgb_backward_splits(8, 32, 1024 * 1024) >= 64          # enough blocks to fill the chip
    assert L.fmgan_torgb_backward_splits(2, 512, 16) == 1
    assert L.fmgan_torgb_backward_splits(2, 512, 18) == 0                   # H*W % 4 != 0: composite instead
    assert L.fmgan_torgb_backward_splits(0, 512, 16) == 0
    assert L.fmgan_torgb_backward_f32(None, None, None, None, None, None, 0, 32, 3, 64, 1.0, None) == 0
    assert L.fmgan_torgb_backward_f32(None, None, None, None, None, None, 2, 32, 3, 64, 1.0, None) == -1
    assert L.fmgan_torgb_backward_f32(16, 16, 16, 16, 16, 16, 2, 32, 5, 64, 1.0, None) == -1     # cout > 4
    assert L.fmgan_torgb_backward_f32(16, 16, 16, 16, 16, 16, 2, 32, 3, 66, 1.0, None) == -2


def test_product_has_no_cpu_path():
    from op import upfirdn2d, fused_leaky_relu, FusedLeakyReLU
    x = torch.randn(1, 2, 8, 8)
    k = cases.make_fir('blur')
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        upfirdn2d(x, k, pad=(1, 1))
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        fused_leaky_relu(x, torch.zeros(2))
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        FusedLeakyReLU(2)(x)
    import stylegan2
    g = stylegan2.Generator(16, 512, 1, generator_net_shape=[8, 8, 8, 8, 8, 8])
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        g(None, latent_styles=[torch.randn(1, g.n_latent, 512)], input_is_latent=True,
          use_external_input_tensor=True, external_input_tensor=torch.randn(1, 8, 4, 4))


def test_raw_pointer_entry_points_refuse_other_dtypes():
    """The f32 entry points take raw pointers; a bf16 / f64 / CPU tensor must be refused on the host (RuntimeError), never
    handed to a kernel that would read past its end (round 3: a bf16 style vector under autocast faulted the GPU)."""
    from op import _native
    assert _native.fp(None) is None
    for t in (torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.float64), torch.zeros(4)):
        with pytest.raises(RuntimeError):
            _native.fp(t)
    for fn in ('modconv2d', 'modconv_demod', 'torgb', 'torgb_backward', 'noise_bias_act', 'blur_noise_bias_act',
               'modconv2d_rgb', 'modconv_wgrad', 'prelu_backward', 'fused_bias_act_backward'):
        body = inspect.getsource(getattr(_native, fn))
        assert ' ptr(' not in body.replace('ptr(wtb)', '').replace('ptr(wts)', '') and 'fp(' in body, fn


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, '3d-fm-gan_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                src = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in src.replace('# oracle', ''), f'{f} mentions the oracle'


def _check_manifest(module, man):
    sd = module.state_dict()
    assert list(sd.keys()) == sorted(sd.keys(), key=list(sd.keys()).index)  # trivial, keeps order explicit
    assert set(sd.keys()) == set(man.keys()), (set(sd.keys()) ^ set(man.keys()))
    for k, shape in man.items():
        assert list(sd[k].shape) == shape, k


def test_generator_state_dict_matches_reference(golden):
    import stylegan2
    man = golden.manifest('generator')
    for c in cases.GENERATOR_CASES:
        if c['size'] > 256:
            continue
        g = stylegan2.Generator(c['size'], 512, c['n_mlp'], generator_net_shape=c['shape'])
        _check_manifest(g, man[c['name']])
        assert g.n_latent == int(torch.log2(torch.tensor(float(c['size'])))) * 2 - 2
    g = stylegan2.Generator(256, 512, 8)
    assert len(g.state_dict()) == 135   # SURVEY.md §5 checkpoint row
    assert tuple(g.state_dict()['conv1.conv.weight'].shape) == (1, 512, 512, 3, 3)


def test_module_state_dicts_match_reference(golden):
    import stylegan2
    man = golden.manifest('modules')
    for c in cases.MODCONV_CASES:
        _check_manifest(stylegan2.ModulatedConv2d(c['cin'], c['cout'], c['k'], 512, demodulate=c['demod'],
                                                  upsample=c['up']), man[c['name']])
    for c in cases.STYLEDCONV_CASES:
        _check_manifest(stylegan2.StyledConv(c['cin'], c['cout'], 3, 512, upsample=c['up']), man[c['name']])
    for c in cases.TORGB_CASES:
        _check_manifest(stylegan2.ToRGB(c['cin'], 512, upsample=c['skip']), man[c['name']])


def test_discriminator_and_encoder_state_dicts_match_reference(golden):
    import types
    import stylegan2
    import resnet_encoder
    from psp_encoder_model.encoders import psp_encoders
    _check_manifest(stylegan2.Discriminator(64), golden.manifest('discriminator')['d64'])
    man = golden.manifest('encoders')
    _check_manifest(resnet_encoder.resnet18(tensor_encoding=True, tensor_transform=False), man['resnet'])
    _check_manifest(resnet_encoder.resnet18(tensor_encoding=False), man['resnet'])
    for n in (14, 18):
        opts = types.SimpleNamespace(input_nc=3, n_styles=n)
        _check_manifest(psp_encoders.GradualStyleEncoder(18, 'ir_se', opts), man[f'psp{n}'])


def test_encoders_match_golden_on_cpu(golden):
    """The encoders are plain PyTorch modules (no custom kernel), so they also run on CPU: check the product's
    modules against the reference's outputs here; the GPU run repeats this on MIOpen."""
    import types
    import numpy as np
    import resnet_encoder
    from psp_encoder_model.encoders import psp_encoders
    g = golden('e2e')
    name = 'e2e_256'
    p = synth.tensor(name + '/photo', (1, 3, 256, 256), dist='uniform')
    r = synth.tensor(name + '/render', (1, 3, 256, 256), dist='uniform')
    e_tsr = resnet_encoder.resnet18(tensor_encoding=True)
    e_w = resnet_encoder.resnet18(tensor_encoding=False)
    e_wp = psp_encoders.GradualStyleEncoder(18, 'ir_se', types.SimpleNamespace(input_nc=3, n_styles=14))
    for kind, m, seed in (('resnet', e_tsr, 5), ('resnet', e_w, 6), ('psp', e_wp, 7)):
        m.load_state_dict(synth.state_dict(kind, m.state_dict(), seed=seed))
        m.eval()
    with torch.no_grad():
        np.testing.assert_allclose(e_tsr(p).numpy(), g[name + '/e_tsr'], atol=2e-4, rtol=2e-4)
        np.testing.assert_allclose(e_w(r).numpy(), g[name + '/e_w'], atol=2e-4, rtol=2e-4)
        ref = g[name + '/e_wplus']
        np.testing.assert_allclose(e_wp(p).numpy(), ref, atol=2e-4 * np.abs(ref).max(), rtol=2e-4)


def test_network_shape_helpers():
    import stylegan2
    from Util import network_util
    shape = [16, 16, 16, 16, 16, 16, 8, 8, 8, 8]
    g = stylegan2.Generator(64, 512, 2, generator_net_shape=shape)
    assert network_util.Get_Network_Shape(g.state_dict()) == shape
    g2 = network_util.Build_Generator_From_Dict(g.state_dict(), size=64, n_mlp=2)
    assert [tuple(v.shape) for v in g2.state_dict().values()] == [tuple(v.shape) for v in g.state_dict().values()]


def test_training_losses_on_cpu_tensors():
    """Util/training_util.py mirrors the reference's GAN losses (training_util.py:24-58): closed forms on CPU tensors."""
    import math
    from Util import training_util as TU
    real, fake = torch.tensor([[0.5], [-1.0]]), torch.tensor([[2.0], [0.0]])
    sp = lambda v: math.log1p(math.exp(v))
    assert abs(TU.d_logistic_loss(real, fake).item() - ((sp(-0.5) + sp(1.0)) / 2 + (sp(2.0) + sp(0.0)) / 2)) < 1e-6
    assert abs(TU.g_nonsaturating_loss(fake).item() - (sp(-2.0) + sp(0.0)) / 2) < 1e-6
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0]], requires_grad=True)
    pred = (x ** 2).sum(1, keepdim=True)                      # d/dx = 2x  ->  R1 = mean_b sum 4 x^2
    r1 = TU.d_r1_loss(pred, x)
    assert abs(r1.item() - (4 * (1 + 4) + 4 * (9 + 16)) / 2) < 1e-5
    r1.backward()                                             # second order: d R1 / dx = 8x / batch
    assert torch.allclose(x.grad, 4 * x.detach())
    lat = torch.ones(2, 3, 4, requires_grad=True)
    img = (lat.sum((1, 2))[:, None, None, None] * torch.ones(2, 1, 2, 2))
    pen, mean, pl = TU.g_path_regularize(img, lat, torch.tensor(0.0), probe=torch.ones_like(img))
    # probe / sqrt(4) = 0.5 per pixel, 4 pixels -> d/dlat = 2 everywhere; length = sqrt(mean_over_latents(sum_512 4))
    assert torch.allclose(pl, torch.full((2,), math.sqrt(4 * 4))) and abs(mean.item() - 0.04) < 1e-6
    assert abs(pen.item() - (4 - 0.04) ** 2) < 1e-4
    assert abs(TU.L1_Loss(torch.zeros(2, 3), torch.full((2, 3), -2.0)).item() - 2.0) < 1e-7


@pytest.mark.skipif(torch.cuda.is_available(), reason='passes fake pointers: host-side guard check for the CPU suite only')
def test_modconv_index_range_guards_refuse_without_launching():
    """Shapes just OUTSIDE each index-range guard of fmgan_modconv2d_f32 / fmgan_modconv_wgrad_f32 return
    FMGAN_EOVERFLOW before anything is launched (the pointers here are fake).  The same guards from the inside —
    shapes just below them must compute correctly — are GPU tests (tests/test_hip_modconv.py::test_guard_boundary_*)."""
    L = lib()
    fake = ctypes.c_void_p(0x1000)
    EOVER, EINVAL = -4, -1

    def conv(batch, cin, cout, h, w, mode):
        return L.fmgan_modconv2d_f32(fake, fake, fake, None, fake, batch, cin, cout, h, w, mode, None, None, None, 1, 0,
                                     0.2, 1.4, 0, 0, None, 0, None)

    # per-tile input offsets are 32-bit: (samples per tile) * cin * h * w must stay below 2^31 elements
    assert conv(1, 8, 8, 16384, 16384, 0) == EOVER            # exactly 2^31
    assert conv(1, 8, 8, 16384, 16384, 1) == EOVER
    assert conv(1, 16, 8, 16384, 8192, 2) == EOVER
    assert conv(1, 2049, 8, 1024, 1024, 0) == EOVER           # 2^31 + 2^20
    # pixel indices y*ow + x are 32-bit
    assert conv(1, 1, 1, 46341, 46341, 0) == EOVER
    assert conv(1, 1, 1, 23171, 23171, 1) == EOVER            # output 46343^2
    # channel counts beyond the 32-bit weight offsets
    assert conv(1, (1 << 20) + 1, 8, 4, 4, 0) == EOVER
    assert conv(1, 8, (1 << 20) + 1, 4, 4, 0) == EOVER
    # whole-output element count
    assert conv(70000, 512, 512, 256, 256, 0) == EOVER
    # and the neighbouring failure classes stay distinct
    assert conv(1, 8, 8, 0, 16, 0) == EINVAL
    assert conv(1, 8, 8, 2, 2, 2) == EINVAL
    assert L.fmgan_modconv_wgrad_f32(fake, None, fake, fake, fake, 1, 8, 8, 46341, 46341, 1.0, fake, 1 << 30, None) == EOVER
    assert L.fmgan_modconv_wgrad_f32(fake, None, fake, fake, fake, 1, (1 << 20) + 1, 8, 32, 32, 1.0, fake, 1 << 30, None) == EOVER


@pytest.mark.parametrize('geom', [(3, 1, 1), (3, 2, 0), (1, 2, 0), (1, 1, 0)])
def test_conv_grad_family_matches_conv2d_autograd_at_every_order(geom):
    """op/conv_grad.py: conv2d as three Functions that differentiate into each other (host logic, library primitives —
    runs on CPU too).  First, second and third order agree with F.conv2d's own autograd on the Discriminator's four
    geometries (3x3 pad 1; 3x3 stride 2; 1x1 stride 2; 1x1), in float64."""
    from op import conv_grad
    k, stride, pad = geom
    torch.manual_seed(3)
    x = torch.randn(2, 3, 9, 8, dtype=torch.float64, requires_grad=True)
    w = torch.randn(4, 3, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.randn(4, dtype=torch.float64, requires_grad=True)

    def ours(x_, w_, b_):
        return conv_grad.conv2d(x_, w_, b_, stride, pad)

    def ref(x_, w_, b_):
        return F.conv2d(x_, w_, b_, stride, pad)
    assert torch.autograd.gradcheck(ours, (x, w, b))
    assert torch.autograd.gradgradcheck(ours, (x, w, b))
    # R1-shaped use: penalty on the input gradient, differentiated w.r.t. the weight — and once more
    outs = []
    for f in (ours, ref):
        y = f(x, w, b)
        gx, = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)
        pen = gx.pow(2).sum()
        gw, = torch.autograd.grad(pen, w, create_graph=True)
        g3, = torch.autograd.grad(gw.pow(2).sum(), x)
        outs.append((y.detach(), gx.detach(), gw.detach(), g3))
    for a, c in zip(*outs):
        torch.testing.assert_close(a, c, rtol=1e-10, atol=1e-10)


def test_live_weights_deepcopy_starts_without_table():
    """copy.deepcopy(G) (how Trainer builds g_ema): the copy's LiveWeights must not inherit the original's device table or
    pointer key (raw pointers of the ORIGINAL's parameters and buffers); it is bound to the copied network."""
    import copy
    import stylegan2
    from op.live_weights import LiveWeights
    G = stylegan2.Generator(8, 16, 1, generator_net_shape=[8, 8, 8])
    lw = LiveWeights(G)
    lw._key, lw._table, lw._n, lw._blocks, lw._buffers = ('stale',), torch.zeros(4), 3, 7, [torch.zeros(1)]
    G._live_weights = lw
    G2 = copy.deepcopy(G)
    lw2 = G2._live_weights
    assert lw2 is not lw and lw2.root is G2
    assert lw2._key is None and lw2._table is None and lw2._buffers == [] and not lw2.active
    assert lw._key == ('stale',)


def test_winograd_selection_rule_is_host_logic():
    """stylegan2.winograd_pays: which plain StyledConv layers take the Winograd F(2x2,3x3) form — wide layers of
    16^2..128^2 with enough tiles, fp32 precision only, even sizes only."""
    import stylegan2
    from op import _native
    assert stylegan2.winograd_pays(8, 512, 512, 64, 64) and stylegan2.winograd_pays(8, 256, 256, 128, 128)
    assert stylegan2.winograd_pays(8, 512, 512, 16, 16) and stylegan2.winograd_pays(32, 512, 512, 16, 16)
    assert not stylegan2.winograd_pays(8, 128, 128, 256, 256)       # transforms cost more than the saved MACs
    assert not stylegan2.winograd_pays(8, 64, 64, 512, 512) and not stylegan2.winograd_pays(8, 512, 512, 8, 8)
    assert not stylegan2.winograd_pays(1, 512, 512, 16, 16)         # 64 tiles: too few columns for the 16 GEMMs
    assert not stylegan2.winograd_pays(8, 512, 512, 63, 64) and not stylegan2.winograd_pays(8, 512, 256, 64, 65)
    with _native.modconv_precision('bf16x3'):
        assert not stylegan2.winograd_pays(8, 512, 512, 64, 64)
    old = stylegan2.WINOGRAD
    try:
        stylegan2.WINOGRAD = False
        assert not stylegan2.winograd_pays(8, 512, 512, 64, 64)
    finally:
        stylegan2.WINOGRAD = old


def test_fused_blur_selection_declines_firs_wider_than_four_taps():
    """fmgan_blur_noise_bias_act_select is host logic: the 4-tap blur of every upsampling layer has a kernel (plane-tile for
    small planes, row-march / LDS-DMA ring for wide ones); a 5-tap FIR such as [1,4,6,4,1] has none, which is the case in
    which _native.blur_noise_bias_act returns None and StyledConv takes the two-pass form (and no placement workspace)."""
    from op import _native
    L = lib()
    for b, c, h in ((8, 512, 17), (8, 256, 129), (8, 32, 1025)):
        _, off, ps, rs = _native.aligned_rows_shape(b, c, h, h, 1)
        assert L.fmgan_blur_noise_bias_act_select(None, None, None, b, c, h, h, ps, rs, 4, 4, 1, 1, 1, 1) in (1, 2, 5)
        assert _native.blur_noise_bias_act_serves(b, c, h, h, ps, rs, (4, 4), (1, 1))
        _, off, ps, rs = _native.aligned_rows_shape(b, c, h, h, 2)
        assert L.fmgan_blur_noise_bias_act_select(None, None, None, b, c, h, h, ps, rs, 5, 5, 2, 1, 2, 1) == -2
        assert not _native.blur_noise_bias_act_serves(b, c, h, h, ps, rs, (5, 5), (2, 1))


def test_upfirdn2d_selects_return_the_launch_status():
    """Both select functions are the launch's own plan with the launch left out: arguments the launch refuses get the
    launch's status, not a kernel id.  Every call here is refused before any HIP call (the pointers are placeholders)."""
    L = lib()
    fake = ctypes.c_void_p(0x1000)
    EINVAL, EOVER = -1, -4

    def fused(b, c, h, w, ps, rs):
        sel = L.fmgan_blur_noise_bias_act_select(None, None, None, b, c, h, w, ps, rs, 4, 4, 1, 1, 1, 1)
        run = L.fmgan_blur_noise_bias_act_path_f32(fake, fake, fake, b, c, h, w, ps, rs, 4, 4, 1, 1, 1, 1, None, None, None, 1,
                                                   0.2, 1.4, -1, None)
        return sel, run
    assert fused(1, 4, 129, 129, 129 * 129, 100) == (EINVAL, EINVAL)             # row stride below in_w
    assert fused(1, 4, 129, 129, 10, 129) == (EINVAL, EINVAL)                    # plane stride below one plane
    assert fused(1, 1, 70000, 129, 70000 * 32768, 32768) == (EOVER, EOVER)       # plane above 2^31 elements
    big = (0, 1, 70000, 40000, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1)                  # f32 [1, 70000, 40000, 1]
    assert L.fmgan_upfirdn2d_select(*big) == EOVER
    assert L.fmgan_upfirdn2d(0, fake, fake, fake, *big[1:], -1, None) == EOVER
    # what the selects answered before for arguments the launch accepts, they still answer
    assert L.fmgan_upfirdn2d_select(0, 256, 1025, 1025, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == 1
    assert L.fmgan_upfirdn2d_select(0, 1024, 9, 9, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) != 1
    assert L.fmgan_upfirdn2d_select(1, 256, 1025, 1025, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == 0
    assert L.fmgan_upfirdn2d_select(0, 1, 0, 8, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == -1
    assert L.fmgan_upfirdn2d_select(7, 1, 8, 8, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == -2
    from op import _native
    for b, c, h in ((8, 512, 17), (8, 256, 129), (8, 32, 1025)):
        _, off, ps, rs = _native.aligned_rows_shape(b, c, h, h, 1)
        assert L.fmgan_blur_noise_bias_act_select(None, None, None, b, c, h, h, ps, rs, 4, 4, 1, 1, 1, 1) == (2 if h < 64 else 1)
        _, off, ps, rs = _native.aligned_rows_shape(b, c, h, h, 2)
        assert L.fmgan_blur_noise_bias_act_select(None, None, None, b, c, h, h, ps, rs, 5, 5, 2, 1, 2, 1) == -2
    assert L.fmgan_blur_noise_bias_act_select(None, None, None, 0, 4, 129, 129, 129 * 129, 129, 4, 4, 1, 1, 1, 1) == EINVAL


def test_upfirdn2d_kernel_case_tables_reach_their_kernels():
    """tests/ufd_cases.py, every row: fmgan_upfirdn2d_select names the kernel the row was written for (1 where the row says
    5: the ring is chosen by address, which this select does not get) and the output has the size the table states.  The
    GPU tests assert the same before they run; here a change of the plan's rules fails without a GPU.  (Without a device
    the plan assumes 256 CUs, the count the two scaled rows were written for.)"""
    import ufd_cases
    from op import _native
    L = lib()
    assert len(set(ufd_cases.ALL_ROWS)) == len(ufd_cases.ALL_ROWS) == len(ufd_cases.OUT_SIZE)
    assert ufd_cases.rowmarch_tall_major(256) == ufd_cases.ROWMARCH_TALL[1]
    assert ufd_cases.up2_trip_major(256) == ufd_cases.UP2_TRIP[1]
    reached = set()
    for row in ufd_cases.ALL_ROWS:
        kernel, major, in_h, in_w, kh, kw, up, px0, px1, py0, py1 = row
        sel = L.fmgan_upfirdn2d_select(0, major, in_h, in_w, 1, kh, kw, up, up, 1, 1, px0, px1, py0, py1)
        assert sel == (1 if kernel == 5 else kernel), f'{ufd_cases.row_id(row)}: select says {sel}'
        assert _native.upfirdn2d_out_size(in_h, in_w, kh, kw, up, up, 1, 1, px0, px1, py0, py1) == ufd_cases.OUT_SIZE[row], row
        reached.add(kernel)
    assert reached == {0, 1, 5, 2, 3}
    assert all(r in ufd_cases.ALL_ROWS for r in ufd_cases.FUSED)
    # each parity instantiation of the up2 kernel has a directed row
    assert {(r[9] & 1, r[7] & 1) for r in ufd_cases.UP2} == {(0, 1), (1, 0), (1, 1)}


def test_bf16_launches_ask_supported():
    """fmgan_modconv2d_bf16(_x3)_supported is the one statement of which shapes the bf16 contractions serve, and the
    launch asks it: for every refused shape, and for mode 2 on the split-operand entry, `_supported` is 0 and the launch
    (placeholder pointers, nothing reaches HIP) returns FMGAN_EUNSUPPORTED."""
    L = lib()
    fake = ctypes.c_void_p(0x1000)
    refused = ((2, 12, 32, 64, 64, 0), (2, 32, 48, 64, 64, 0), (2, 32, 32, 16, 16, 0), (2, 512, 512, 4, 4, 1),
               (1, 32, 32, 40, 40, 2))
    for name, cfgs in (('bf16', refused), ('bf16x3', refused + ((2, 32, 32, 65, 65, 2),))):
        supported, launch = getattr(L, f'fmgan_modconv2d_{name}_supported'), getattr(L, f'fmgan_modconv2d_{name}')
        for cfg in cfgs:
            assert supported(*cfg) == 0, (name, cfg)
            assert launch(fake, fake, fake, None, fake, *cfg, None, None, None, 1, 0, 0.2, 1.4, 0, 0, None) == -2, (name, cfg)
    assert L.fmgan_modconv2d_bf16_supported(2, 32, 32, 65, 65, 2) == 1          # mode 2 is the bf16 entry's alone


# ------------------------------------------------------------------------ fmgan_modconv2d_select / fmgan_modconv2d_tiles
def test_modconv_select_and_tiles_are_host_logic():
    """Which tile, which split: both answers come without a device, invalid arguments return the launch's status, the tile
    table lists one tile per (mode, cfg, letter) with the channel extent of its class, and the split reported is the one
    fmgan_modconv2d_workspace_bytes sizes the workspace for."""
    from op import _native
    L = lib()
    tiles = _native.modconv2d_tiles()
    assert L.fmgan_modconv2d_tiles(None, 0) == len(tiles) == 16
    assert len({t[:3] for t in tiles}) == len(tiles)
    for mode, cfg, variant, bm, bn, rgb in tiles:
        assert mode in (0, 1, 2) and bm == (128, 64, 32)[cfg] and bn in (128, 256) and variant in 'ABCDE'
        assert not rgb or mode == 0                                   # the RGB epilogue belongs to the plain conv
        assert (mode, cfg, 'A', bm, 128) in {t[:5] for t in tiles}   # every class has its register tile, the fall-back
    few = (ctypes.c_int * 12)()
    assert L.fmgan_modconv2d_tiles(few, 2) == 16 and tuple(few[:6]) == (0, 0, ord('C'), 128, 256, 0)

    def status(*args):
        return L.fmgan_modconv2d_select(*args, None, None, None, None, None)
    assert status(1, 8, 8, 4, 4, 3, 0, 1) == -2                      # as fmgan_modconv2d_f32: unknown mode
    assert status(1, 8, 8, 0, 4, 0, 0, 1) == -1
    assert status(1, 0, 8, 4, 4, 0, 0, 1) == -1
    assert status(1, 8, 8, 2, 2, 2, 0, 1) == -1                      # stride-2 conv of an image smaller than its window
    assert status(1, 8, 8, 16384, 16384, 0, 0, 1) == -4              # 32-bit per-tile offsets
    assert status(1, 256, 256, 128, 128, 0, 1, 1) == -2              # as fmgan_modconv2d_rgb_f32: not fusable
    assert status(8, 32, 32, 64, 64, 1, 1, 1) == -2                  # the fused launch is the plain conv's
    assert status(0, 8, 8, 4, 4, 0, 0, 1) == 0                       # empty batch: nothing to launch
    with pytest.raises(RuntimeError):
        _native.modconv2d_select(1, 8, 8, 4, 4, 3)
    assert _native.modconv2d_select(0, 8, 8, 4, 4, 0) == (-1, '', 0, 0, 0)
    by_key = {t[:3]: t for t in tiles}
    for mode in (0, 1, 2):
        for b, cin, cout, h, w in ((1, 512, 512, 5, 5), (8, 512, 512, 16, 16), (2, 64, 200, 33, 31), (4, 128, 64, 32, 32),
                                   (8, 32, 32, 1024, 1024), (3, 20, 40, 257, 34), (2, 256, 64, 129, 131), (1, 8, 3, 7, 9)):
            cfg, variant, bm, bn, ks = _native.modconv2d_select(b, cin, cout, h, w, mode)
            assert by_key[(mode, cfg, variant)][3:5] == (bm, bn)
            oh, ow = (2 * h + 1, 2 * w + 1) if mode == 1 else (((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == 2 else (h, w))
            need = L.fmgan_modconv2d_workspace_bytes(b, cin, cout, h, w, mode)
            assert need == (ks * b * cout * oh * ow * 4 if ks > 1 else 0), (mode, b, cin, cout, h, w, ks, need)
            assert _native.modconv2d_select(b, cin, cout, h, w, mode, has_workspace=False)[4] == 1   # no workspace: unsplit
    assert any(_native.modconv2d_select(b, 512, 512, 8, 8, 0)[4] > 1 for b in (1, 8))


def test_modconv_wgrad_select_is_host_logic_and_sizes_the_workspace():
    """fmgan_modconv_wgrad_select answers without a device, returns the launch's status for arguments the launch refuses,
    and names the split that fmgan_modconv_wgrad_mode_workspace_bytes sizes the workspace for — on served and on declined
    shapes alike (the three entry points call one plan function)."""
    from op import _native
    L = lib()

    def status(*args):
        return L.fmgan_modconv_wgrad_select(*args, None, None, None, None, None, None, None)
    assert status(1, 64, 64, 16, 16, 3, 1) == -2                     # as fmgan_modconv_wgrad_mode_f32: unknown mode
    assert status(0, 64, 64, 16, 16, 0, 1) == -1 and status(1, 64, 0, 16, 16, 0, 1) == -1
    assert status(1, 8, 8, 46341, 46341, 0, 1) == -4                 # 32-bit pixel indices
    assert status(1, (1 << 20) + 1, 8, 32, 32, 0, 1) == -4
    assert status(1, 64, 64, 16, 15, 0, 1) == -2 and status(1, 64, 64, 16, 16, 0, 1) == 0
    with pytest.raises(RuntimeError):
        _native.modconv_wgrad_select(1, 8, 8, 46341, 46341)
    assert _native.modconv_wgrad_select(1, 64, 64, 16, 16, 3) == (0, 0, 0, 0, 0, 0, False)
    seen = set()
    for mode in (0, 1, 2):
        for b in (1, 2, 8):
            for cin, cout in ((3, 33), (47, 47), (48, 47), (47, 48), (48, 48), (64, 32), (100, 50), (512, 512), (512, 40)):
                for h, w in ((1, 16), (2, 15), (4, 16), (5, 33), (9, 31), (16, 32), (18, 32), (33, 35), (64, 64), (6, 36)):
                    family, tw, sp, ks, tps, ntiles, vec = sel = _native.modconv_wgrad_select(b, cin, cout, h, w, mode)
                    need = L.fmgan_modconv_wgrad_mode_workspace_bytes(b, cin, cout, h, w, mode)
                    assert need == ks * 9 * cout * cin * 4, (mode, b, cin, cout, h, w, sel, need)
                    wa = w if mode < 2 else (w - 3) // 2 + 1
                    if family == 0:
                        assert sel == (0, 0, 0, 0, 0, 0, False)
                        assert wa < 16 or (mode == 2 and h < 3) or (mode > 0 and min(cin, cout) < 48), (mode, cin, cout, h, w)
                        continue
                    assert family == (64 if min(cin, cout) >= 48 else 32) and (family == 64 or mode == 0)
                    assert sp == (1 if mode == 0 else 2) and tw == (32 if mode == 0 and wa >= 32 else 16)
                    assert ks >= 1 and (ks - 1) * tps < ntiles <= ks * tps       # no empty split; the last may be shorter
                    assert vec == (family == 64 and wa % 4 == 0)
                    unaligned = _native.modconv_wgrad_select(b, cin, cout, h, w, mode, aligned16=False)
                    assert unaligned == sel[:6] + (False,)                       # alignment moves the staging path only
                    seen.add((family, tw, sp, vec))
    assert seen == {(32, 16, 1, False), (32, 32, 1, False), (64, 32, 1, True), (64, 32, 1, False), (64, 16, 1, True),
                    (64, 16, 1, False), (64, 16, 2, True), (64, 16, 2, False)}


def test_modconv_select_headline_forward_dispatch():
    """The documented dispatch of the batch-8 1024^2 forward (csrc/modconv_fwd.hip, the comment block above MC_TILES and
    launch_any; network widths 512 / 256 / 128 / 64 / 32 at 64^2 .. 1024^2), derived from those comments, not recorded:
    Cout >= 96 -> the 128 x 256 tile 'C', Cout >= 48 -> 64 x 256 'C', below -> 32 x 256 'E', all unsplit; a fused-ToRGB
    launch of the 128- and 64-channel classes never takes 'C' but the register tile 'A', the 32-channel class keeps 'E';
    at batch 1 the 64^2 .. 256^2 layers have too few 256-position tiles to fill the chip twice and take 'B'."""
    from op import _native
    widths = {64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}

    def sel(b, r, rgb=False):
        c = widths[r]
        return _native.modconv2d_select(b, c, c, r, r, 0, rgb=rgb)
    for r in (64, 128, 256):
        assert sel(8, r) == (0, 'C', 128, 256, 1), r
        assert sel(1, r)[:4] == (0, 'B', 128, 128), r
    assert sel(8, 512) == (1, 'C', 64, 256, 1)
    assert sel(8, 1024) == (2, 'E', 32, 256, 1) and sel(8, 1024, rgb=True) == (2, 'E', 32, 256, 1)
    assert sel(8, 256, rgb=True) == (0, 'A', 128, 128, 1) and sel(8, 512, rgb=True) == (1, 'A', 64, 128, 1)
    for r in (64, 128):                                             # two and more channel tiles: not fusable
        assert not _native.modconv2d_rgb_fusable(8, widths[r], widths[r], r, r)
        with pytest.raises(RuntimeError):
            sel(8, r, rgb=True)


def test_modconv_select_keeps_fused_torgb_on_single_sample_tiles():
    """fmgan_modconv2d_rgb_fusable answers on the 128-position planning model; a 256-position tile packs two samples of a
    4-row image (TW = 32: 8 rows per tile) or an 8-row, 16-wide image into one tile, and the RGB epilogue reads one sample's
    weights per block: such a fused launch takes the register tile, the unfused one keeps 'E'."""
    from op import _native
    for shape in ((16, 8, 32, 4, 2048), (1024, 8, 32, 8, 16)):
        assert _native.modconv2d_rgb_fusable(*shape)
        assert _native.modconv2d_select(*shape, 0) == (2, 'E', 32, 256, 1)
        assert _native.modconv2d_select(*shape, 0, rgb=True) == (2, 'A', 32, 128, 1)
    assert _native.modconv2d_select(16, 8, 32, 8, 2048, 0, rgb=True) == (2, 'E', 32, 256, 1)     # 8 rows fill the tile
