"""CPU tests of the 16-bit activation path (csrc/act16.hip): the new symbols are declared, exported and
described; the select / blocks queries answer without a GPU and bad arguments are refused before any HIP call; the new
kernels keep 8 waves per SIMD without spilling; the fragments tests/test_kernel_budgets.py looks kernels up by still hit
one kernel each; and the training program's --precision / --bf16_io arguments and the FMGAN_NO_BF16_IO switch."""
import os
import re
import types

import pytest
import torch

import codeobj
import test_kernel_budgets as budgets
from nets import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('fmgan_act16_fba_select', 'fmgan_act16_fba', 'fmgan_act16_fba_bwd_blocks', 'fmgan_act16_fba_bwd',
           'fmgan_ufd16_select', 'fmgan_ufd16')
F32, F64, F16, BF16 = 0, 1, 2, 3
EINVAL, EUNSUPPORTED, EOVERFLOW = -1, -2, -4
AUTOCAST = torch.cuda.is_available()       # torch.autocast('cuda') switches itself off (with a warning) without a GPU
P = 4096        # any even non-null address: every refusal below happens before a pointer is used or a HIP call is made


def test_symbols_are_declared_exported_and_described():
    hdr = open(os.path.join(ROOT, 'include', 'fmgan_hip.h')).read()
    assert re.search(r'#define\s+FMGAN_BF16\s+3\b', hdr) and re.search(r'#define\s+FMGAN_F16\s+2\b', hdr)
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    L = lib()
    for n in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % n, hdr), f'{n} is not declared in include/fmgan_hip.h'
        assert hasattr(L, n), f'{n} is not exported'
        assert n in doc, f'{n} is not described in INTEGRATION.md'
    assert L.fmgan_abi_version() == 1
    from op import _native
    assert (_native.F16, _native.BF16) == (F16, BF16)


def test_fba_select_and_refusals():
    L = lib()
    sel = L.fmgan_act16_fba_select
    for dt in (F16, BF16):
        assert sel(dt, 2 * 3 * 45, 3, 45, 3, 0) == 1          # planes, bias per plane
        assert sel(dt, 4 * 512, 512, 1, 3, 1) == 2            # bias innermost
        assert sel(dt, 100, 0, 7, 1, 0) == 3                  # no bias: one run
        assert sel(dt, 0, 0, 1, 3, 0) == 3                    # an empty tensor is a no-op for the launch
        for act, grad in ((1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2)):
            assert sel(dt, 90, 3, 15, act, grad) == 1
        assert sel(dt, 90, 3, 15, 2, 0) == EUNSUPPORTED and sel(dt, 90, 3, 15, 3, 3) == EUNSUPPORTED
        assert sel(dt, 91, 3, 15, 3, 0) == EINVAL             # not a whole number of planes
        assert sel(dt, -1, 3, 15, 3, 0) == EINVAL and sel(dt, 90, -1, 15, 3, 0) == EINVAL
        assert sel(dt, 90, 3, 0, 3, 0) == EINVAL
        assert sel(dt, 1 << 32, 4, 1, 3, 0) == EOVERFLOW      # the bias-innermost kernel indexes with 31 bits
    assert sel(F32, 90, 3, 15, 3, 0) == EUNSUPPORTED and sel(F64, 90, 3, 15, 3, 0) == EUNSUPPORTED

    def fba(dtype=BF16, x=P, bias=P, ref=None, out=P, n=90, size_b=3, step_b=15, act=3, grad=0):
        return L.fmgan_act16_fba(dtype, x, bias, ref, out, n, size_b, step_b, act, grad, 0.2, 1.0, None)

    assert fba(dtype=F32) == EUNSUPPORTED
    assert fba(x=None) == EINVAL and fba(out=None) == EINVAL
    assert fba(x=P + 1) == EINVAL and fba(out=P + 1) == EINVAL and fba(ref=P + 1) == EINVAL   # 2-byte elements
    assert fba(bias=P + 2) == EINVAL                                                          # fp32 bias
    assert fba(n=91) == EINVAL and fba(act=2) == EUNSUPPORTED
    assert fba(n=0) == 0 and fba(n=0, x=None, out=None) == 0


def test_fba_bwd_blocks_and_refusals():
    L = lib()
    blocks = L.fmgan_act16_fba_bwd_blocks
    assert blocks(6, 1) == 1 and blocks(6, 8192) == 1 and blocks(6, 8193) == 2
    assert blocks(256, 1024 * 1024) == 64                     # capped: 64 partial sums per plane
    assert blocks(0, 64) == 0 and blocks(-1, 64) == 0 and blocks(6, 0) == 0 and blocks(1 << 31, 64) == 0

    def bwd(dtype=BF16, g=P, ref=P, gi=P, partial=P, planes=6, hw=45):
        return L.fmgan_act16_fba_bwd(dtype, g, ref, gi, partial, planes, hw, 0.2, 1.0, None)

    assert bwd(dtype=F32) == EUNSUPPORTED and bwd(dtype=F64) == EUNSUPPORTED
    for name in ('g', 'ref', 'gi', 'partial'):
        assert bwd(**{name: None}) == EINVAL, name
    for name in ('g', 'ref', 'gi'):
        assert bwd(**{name: P + 1}) == EINVAL, name
    assert bwd(partial=P + 2) == EINVAL
    assert bwd(planes=-1) == EINVAL and bwd(hw=0) == EINVAL
    assert bwd(planes=1 << 31) == EOVERFLOW
    assert bwd(planes=0) == 0


def test_ufd16_select_and_refusals():
    L = lib()
    sel = L.fmgan_ufd16_select
    for dt in (F16, BF16):
        # the Discriminator's blurs and their backwards: the FIR kernel
        for pad in ((2, 2), (1, 1), (2, 1), (0, 0), (-1, -1), (3, 0)):
            assert sel(dt, 6, 33, 65, 1, 4, 4, 1, 1, 1, 1, pad[0], pad[1], pad[0], pad[1]) == 1, pad
        for kh, kw in ((1, 1), (2, 2), (4, 4), (1, 4), (4, 1), (3, 3)):
            assert sel(dt, 6, 9, 63, 1, kh, kw, 1, 1, 1, 1, 2, 2, 2, 2) == 1
        # everything else: one output per thread
        assert sel(dt, 6, 9, 63, 1, 4, 4, 2, 2, 1, 1, 2, 1, 2, 1) == 0      # up
        assert sel(dt, 6, 9, 63, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1) == 0      # down
        assert sel(dt, 6, 9, 63, 3, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1) == 0      # minor
        assert sel(dt, 6, 9, 63, 1, 5, 5, 1, 1, 1, 1, 2, 2, 2, 2) == 0      # more than 4 taps
        assert sel(dt, 6, 0, 63, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) == EINVAL
        assert sel(dt, 6, 9, 63, 1, 4, 4, 0, 1, 1, 1, 2, 2, 2, 2) == EINVAL
        assert sel(dt, 6, 2, 2, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0) == EINVAL  # empty output
        assert sel(dt, -1, 9, 63, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) == EINVAL
        assert sel(dt, 1, 1 << 16, 1 << 15, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) == EOVERFLOW
    assert sel(F32, 6, 9, 63, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2) == EUNSUPPORTED

    def ufd(dtype=BF16, x=P, k=P, out=P, major=6):
        return L.fmgan_ufd16(dtype, x, k, out, major, 9, 63, 1, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, None)

    assert ufd(dtype=F64) == EUNSUPPORTED
    assert ufd(x=None) == EINVAL and ufd(k=None) == EINVAL and ufd(out=None) == EINVAL
    assert ufd(x=P + 1) == EINVAL and ufd(out=P + 1) == EINVAL and ufd(k=P + 2) == EINVAL
    assert ufd(major=0) == 0


def test_wrappers_have_no_cpu_path():
    from op import _native, fused_leaky_relu, upfirdn2d
    x = torch.zeros(1, 2, 4, 4, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        fused_leaky_relu(x, torch.zeros(2))
    with pytest.raises(RuntimeError):
        upfirdn2d(x, torch.ones(2, 2), pad=(1, 0))
    with pytest.raises(RuntimeError):
        _native.fused_bias_act16(x, torch.zeros(2), None, 3, 0, 0.2, 1.0)
    with pytest.raises(RuntimeError):
        _native.fused_bias_act16_backward(x, x, 0.2, 1.0)
    with pytest.raises(RuntimeError):
        _native.upfirdn2d16(x.reshape(2, 4, 4, 1), torch.ones(2, 2), 1, 1, 1, 1, 1, 0, 1, 0)


def test_activation_io_switch():
    from op import _native
    assert _native.current_activation_io() == 'fp32' and _native.activation._act_io == 'fp32'
    h, b, f = (torch.zeros(1, dtype=d) for d in (torch.float16, torch.bfloat16, torch.float32))
    assert _native.io16(b) and not _native.io16(h) and not _native.io16(f)
    with _native.activation_io('16'):
        assert _native.current_activation_io() == '16' and _native.activation._act_io == '16'
        assert _native.io16(b) and _native.io16(h) and not _native.io16(f)
        with _native.activation_io('fp32'):
            assert _native.current_activation_io() == 'fp32'
        assert _native.current_activation_io() == '16'
    assert _native.current_activation_io() == 'fp32'
    with pytest.raises(ValueError):
        _native.activation_io('bf16')
    with pytest.raises(RuntimeError):
        with _native.activation_io('16'):
            raise RuntimeError('x')
    assert _native.current_activation_io() == 'fp32'


def test_amp_fwd_io_sets_the_fields_that_custom_bwd_reads():
    """_native.amp_fwd_io, on its 16-bit branch, leaves on ctx by hand what torch.amp.custom_fwd leaves there for
    custom_bwd.  This pins those names against the installed torch: custom_fwd sets exactly these two, and custom_bwd
    reads them and nothing else."""
    class Ctx:
        pass
    fwd = torch.amp.custom_fwd(lambda ctx, x: x, device_type='cpu', cast_inputs=torch.float32)
    ctx = Ctx()
    with torch.autocast('cpu', dtype=torch.bfloat16):
        fwd(ctx, torch.zeros(1))
    assert vars(ctx) == {'_dtype': torch.bfloat16, '_fwd_used_autocast': False}
    bwd = torch.amp.custom_bwd(lambda ctx, g: torch.is_autocast_enabled('cpu'), device_type='cpu')
    by_hand = Ctx()
    by_hand._dtype, by_hand._fwd_used_autocast = torch.bfloat16, False
    with torch.autocast('cpu', dtype=torch.bfloat16):
        assert bwd(by_hand, torch.zeros(1)) is False
    with pytest.raises(AttributeError):
        bwd(Ctx(), torch.zeros(1))


# ------------------------------------------------------------------------------------------------- code object
@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    return codeobj.kernel_notes(tmp_path_factory.mktemp('codeobj'))


def test_new_kernels_keep_eight_waves_per_simd(kernels):
    """<= 64 VGPRs (512 / 64 = 8 waves per SIMD), no vector or scalar register spilled, no scratch."""
    new = {n: k for n, k in kernels.items() if 'act16_' in n or 'ufd16_' in n}
    want = {'act16_fbaI': 6, 'act16_fba_innerI': 6, 'act16_fba_bwdI': 2, 'ufd16_firI': 2, 'ufd16_genericI': 2}
    for frag, count in want.items():
        assert sum(frag in n for n in new) == count, (frag, sorted(new))
    assert len(new) == sum(want.values()), sorted(new)
    for name, k in sorted(new.items()):
        print(name, k)
        assert k['vgpr'] <= 64 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0, (name, k)
        assert k['lds'] == (16 if 'act16_fba_bwd' in name else 0), (name, k)


def test_fragments_of_the_budget_tests_still_hit_one_kernel(kernels):
    needles = [m[0] for m in budgets.MODCONV] + [
        'ufd_dmaring_f32ILb1ELb0ELb0E', 'ufd_rowmarch_f32ILi4ELb1E', 'noise_bias_act_f32', 'equal_linear_f32',
        'modconv_demod_f32ILb1E', 'fba_f32_inner4ILi30ELb0E']
    for needle in needles:
        hits = [k for k in kernels if needle in k]
        assert len(hits) == 1, (needle, hits)
    assert sum('modconv_mfma_bf16' in k for k in kernels) == 8
    # none of the new names contains a fragment another test file searches for
    for frag in ('fba_f32', 'ufd_', 'train_ema', 'train_loss_row', 'lbfgs', 'lpips', 'modconv', 'equal_linear'):
        assert not [k for k in kernels if ('act16_' in k or 'ufd16_' in k) and frag in k], frag


# ------------------------------------------------------------------------------------------------- training program
def test_precision_arguments():
    import train_3_encoder as T
    a = T.Args_Parsing([])
    assert a.precision == 'fp32' and a.bf16_io == T.BF16_IO_DEFAULT
    assert T.training_precision(a) == ('fp32', False)
    a = T.Args_Parsing(['--precision', 'bf16', '--bf16_io', 'true'])
    assert (a.precision, a.bf16_io) == ('bf16', True) and T.training_precision(a) == ('bf16', True)
    a = T.Args_Parsing(['--precision', 'bf16', '--bf16_io', 'false'])
    assert T.training_precision(a) == ('bf16', False)
    for bad in ('fp16', 'bfloat16', 'FP32', ''):
        with pytest.raises(SystemExit):
            T.Args_Parsing(['--precision', bad])
    with pytest.raises(SystemExit):
        T.Args_Parsing(['--bf16_io', 'maybe'])
    # default_args() sets neither field: a Trainer built from it trains in fp32, in no context at all
    d = T.default_args()
    assert not hasattr(d, 'precision') and not hasattr(d, 'bf16_io')
    assert T.training_precision(d) == ('fp32', False)
    with pytest.raises(ValueError):
        T.training_precision(types.SimpleNamespace(precision='fp16'))
    # bf16_io does nothing without bf16
    assert T.training_precision(types.SimpleNamespace(precision='fp32', bf16_io=True)) == ('fp32', False)


@pytest.mark.filterwarnings('ignore:CUDA is not available')
def test_precision_context_sets_the_three_switches():
    import train_3_encoder as T
    from op import _native

    def state():
        return (torch.is_autocast_enabled('cuda'), _native.current_modconv_precision(), _native.current_activation_io())

    with T.precision_context(T.default_args()):
        assert state() == (False, 'f32', 'fp32')
    with T.precision_context(types.SimpleNamespace(precision='bf16', bf16_io=True)):
        assert state() == (AUTOCAST, 'bf16', '16') and torch.get_autocast_dtype('cuda') == torch.bfloat16
    with T.precision_context(types.SimpleNamespace(precision='bf16', bf16_io=False)):
        assert state() == (AUTOCAST, 'bf16', 'fp32')
    assert state() == (False, 'f32', 'fp32')


@pytest.mark.filterwarnings('ignore:CUDA is not available')
def test_no_bf16_io_switch(monkeypatch):
    """FMGAN_NO_BF16_IO=1 forces activation_io('fp32') whatever --bf16_io says (read at every step)."""
    import train_3_encoder as T
    from op import _native
    seen = []
    monkeypatch.setattr(T, 'accumulate', lambda *a: seen.append((torch.is_autocast_enabled('cuda'),
                                                                 _native.current_modconv_precision(),
                                                                 _native.current_activation_io())))
    stub = type('S', (), {})()
    stub.args = T.default_args(ema_fuse=False, d_reg_every=10 ** 9, use_g_reg=False)
    stub.args.precision, stub.args.bf16_io = 'bf16', True
    stub.nets = dict.fromkeys(('G', 'E_Tsr', 'E_W', 'E_W_Plus', 'D'))
    stub.bare, stub.g_ema, stub.accum, stub.ema_plan, stub.loss_dict, stub.iter_idx = {'G': None}, None, 0.9, None, {}, 1
    stub.discriminator = lambda ds_flag: (None, None)
    stub.lpips_model = stub.face_rec_model = stub.fa_model = stub.g_enc_optim = None
    monkeypatch.setattr(T, 'D_Loss_BackProp', lambda *a, **k: None)
    monkeypatch.setattr(T, 'G_Loss_BackProp', lambda *a, **k: None)
    T.Trainer.step(stub, None, None, None)
    monkeypatch.setenv('FMGAN_NO_BF16_IO', '1')
    assert T.training_precision(stub.args) == ('bf16', False)
    T.Trainer.step(stub, None, None, None)
    monkeypatch.delenv('FMGAN_NO_BF16_IO')
    stub.args.bf16_io = False
    T.Trainer.step(stub, None, None, None)
    del stub.args.precision, stub.args.bf16_io
    T.Trainer.step(stub, None, None, None)
    assert seen == [(AUTOCAST, 'bf16', '16'), (AUTOCAST, 'bf16', 'fp32'), (AUTOCAST, 'bf16', 'fp32'), (False, 'f32', 'fp32')]


def test_status_text_appends_the_precision_line():
    import train_3_encoder as T
    assert T.Precision_Status_Text(T.default_args()) == ''
    assert T.Precision_Status_Text(types.SimpleNamespace(precision='fp32', bf16_io=True)) == '  Precision: fp32\n\n'
    assert T.Precision_Status_Text(types.SimpleNamespace(precision='bf16', bf16_io=True)) == \
        '  Precision: bf16 (16-bit activation kernels: on)\n\n'
    assert T.Precision_Status_Text(types.SimpleNamespace(precision='bf16', bf16_io=False)) == \
        '  Precision: bf16 (16-bit activation kernels: off)\n\n'
