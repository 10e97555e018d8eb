"""GPU tests of the training loop's two kernels (csrc/train_loop.hip), of op.ema.EmaPlan, and of train() / main() over the
smallest Trainer the suite builds (tests/test_checkpoint_gpu.py: Generator(64, 512, n_mlp=2), B = 2).

The EMA bound.  With dec = float32(decay) and al = float32(1 - decay), the float64 value dec * d + al * s is the
reference, and every element must lie within 2^-23 (|dec d| + |al s|) + 2^-148 of it: the two roundings of either
permitted form (fma(al, s, round(dec d)), or round(round(dec d) + round(al s))) are each at most half an ulp of a
value no larger than |dec d| + |al s|, plus one subnormal step.  The composite (`accumulate`) obeys the same bound, so the
two lie within twice that of each other.  C = 4096 is the kernel's chunk (one block)."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import gpumem
import launches
from gpumem import dev
from nets import lib, load

pytestmark = pytest.mark.gpu
DECAYS = (0.5 ** (32 / 10000), 0.999, 0.0, 1.0)


def _chunk():
    from op import _native
    return _native.EMA_CHUNK


def _values(n, seed):
    """n float32 values of both signs over 40 binades."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(n, generator=g, dtype=torch.float64) * 40 - 30)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def _guarded(n, shift):
    """(buf, view): a float32 view of n elements `shift` floats past a 16-byte boundary, between sentinel words."""
    buf, view = gpumem.guarded(n + shift)
    assert view.data_ptr() % 16 == 0
    if shift:
        buf[gpumem.GUARD:gpumem.GUARD + shift] = gpumem.SENTINEL
    return buf, view[shift:]


class Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.p = torch.nn.ParameterList([torch.nn.Parameter(t, requires_grad=False) for t in tensors])


def _bound(d64, s64, decay):
    dec, al = float(np.float32(decay)), float(np.float32(1.0 - decay))
    ref = dec * d64 + al * s64
    return ref, 2.0 ** -23 * ((dec * d64).abs() + (al * s64).abs()) + 2.0 ** -148


def _run_ema(sizes, decay, dst_shift=0, src_shift=0, seed=0):
    """The kernel over one table of tensors of `sizes`; checks every element against float64 and `accumulate`, and the
    sentinels around every dst."""
    from op import _native, ema
    from Util.training_util import accumulate
    bufs, dsts, srcs, d0 = [], [], [], []
    for k, n in enumerate(sizes):
        buf, d = _guarded(n, dst_shift)
        d.copy_(_values(n, 100 * seed + 2 * k))
        store = torch.empty(n + 4, dtype=torch.float32, device=dev())
        assert store.data_ptr() % 16 == 0
        s = store[src_shift:src_shift + n]
        s.copy_(_values(n, 100 * seed + 2 * k + 1))
        assert d.data_ptr() % 16 == 4 * dst_shift and (n == 0 or s.data_ptr() % 16 == 4 * src_shift)
        bufs.append(buf)
        dsts.append(d)
        srcs.append(s)
        d0.append(d.clone())
    composite = Bag([t.clone() for t in d0])
    accumulate(composite, Bag(srcs), decay)
    table, n_entries, blocks, numel = ema.table_for(list(zip(dsts, srcs)))
    assert blocks == sum(-(-n // _chunk()) for n in sizes)
    with launches.observed() as rec:
        _native.ema(table, n_entries, blocks, decay, numel)
    torch.cuda.synchronize()
    assert rec.names == ['ema']
    worst = 0.0
    for buf, d, s, before, comp in zip(bufs, dsts, srcs, d0, composite.p):
        assert gpumem.guards_intact(buf)
        if dst_shift:
            assert bool((buf[gpumem.GUARD:gpumem.GUARD + dst_shift] == gpumem.SENTINEL).all())
        if d.numel() == 0:
            continue
        ref, bound = _bound(before.double(), s.double(), decay)
        err = (d.double() - ref).abs()
        assert bool((err <= bound).all()), (sizes, decay, float((err / bound).max()))
        assert bool(((d.double() - comp.double()).abs() <= 2 * bound).all()), (sizes, decay)
        worst = max(worst, float((err / bound).max()))
        if decay == 0.0:
            assert torch.equal(d, s)
        if decay == 1.0:
            assert torch.equal(d, before)
    return worst


def test_ema_single_tensor_sizes():
    c = _chunk()
    worst = 0.0
    for n in (1, 3, 4, 5, c - 1, c, c + 1, 2 * c - 1):
        for j, decay in enumerate(DECAYS):
            worst = max(worst, _run_ema([n], decay, seed=j))
    print(f'EMA worst error / bound {worst:.3f}')


def test_ema_table_of_mixed_sizes():
    """Block-to-entry boundaries, a one-element tensor between large ones, an empty tensor."""
    c = _chunk()
    for j, decay in enumerate(DECAYS):
        _run_ema([2 * c + 3, 1, 0, c, 1, 5], decay, seed=10 + j)


@pytest.mark.parametrize('shifts', [(1, 0), (0, 1), (1, 1), (3, 3), (2, 3)], ids=lambda s: f'dst{s[0]}_src{s[1]}')
def test_ema_views_off_a_16_byte_boundary(shifts):
    """dst only, src only, both by the same amount (scalar head, vector body) and by different amounts (all scalar)."""
    c = _chunk()
    for j, decay in enumerate(DECAYS):
        _run_ema([2 * c + 3, 5, c + 1], decay, dst_shift=shifts[0], src_shift=shifts[1], seed=20 + j)


# ------------------------------------------------------------------------------------------------------- EmaPlan
@pytest.fixture(scope='module')
def generators():
    import stylegan2
    G = load(stylegan2.Generator(64, 512, 2), 'generator', 4)
    g_ema = load(stylegan2.Generator(64, 512, 2), 'generator', 9)
    return G, g_ema


def _check_update(plan, g_ema, G, decay):
    from op import _native
    before = {k: p.detach().clone() for k, p in g_ema.named_parameters()}
    buffers = {k: b.clone() for k, b in g_ema.named_buffers()}
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    L = _native.lib()
    real, streams = L.fmgan_ema_f32, []

    def spy(table, n, blocks, dec, al, stream):
        streams.append(stream)
        return real(table, n, blocks, dec, al, stream)
    L.fmgan_ema_f32 = spy
    try:
        with launches.observed() as rec, torch.cuda.stream(side):
            plan.update(decay)
    finally:
        L.fmgan_ema_f32 = real
    assert L.fmgan_ema_f32.argtypes is not None
    assert rec.count('ema') == 1 and rec.names == ['ema']               # one bracket, nothing else launched
    assert streams == [side.cuda_stream] and side.cuda_stream != torch.cuda.current_stream(dev()).cuda_stream
    side.synchronize()
    src = dict(G.named_parameters())
    assert len(before) >= 60
    for k, p in g_ema.named_parameters():
        ref, bound = _bound(before[k].double(), src[k].detach().double(), decay)
        assert bool(((p.detach().double() - ref).abs() <= bound).all()), k
    moved = sum(not torch.equal(p.detach(), before[k]) for k, p in g_ema.named_parameters())
    assert moved > len(before) // 2
    for k, b in g_ema.named_buffers():
        assert torch.equal(b, buffers[k]), k
    assert len(buffers) >= 1


def test_ema_plan_on_a_generator(generators):
    from op.ema import EmaPlan
    G, g_ema = generators
    assert EmaPlan.declined(g_ema, G) is None
    plan = EmaPlan(g_ema, G)
    _check_update(plan, g_ema, G, 0.5 ** (32 / 10000))
    assert plan.rebuilds == 1
    g_ema.load_state_dict({k: v.clone() for k, v in g_ema.state_dict().items()})      # copies in place: same pointers
    _check_update(plan, g_ema, G, 0.999)
    assert plan.rebuilds == 1
    old = [p.data_ptr() for p in g_ema.parameters()]
    g_ema.to(torch.float64).to(torch.float32)
    assert [p.data_ptr() for p in g_ema.parameters()] != old
    _check_update(plan, g_ema, G, 0.999)                                              # re-validated, rebuilt, still right
    assert plan.rebuilds == 2


def test_accumulate_fused_returns_its_plan_and_falls_back(generators):
    from op.ema import EmaPlan
    from Util.training_util import accumulate_fused
    G, g_ema = generators
    with launches.observed() as rec:
        plan = accumulate_fused(g_ema, G, 0.999)
        assert isinstance(plan, EmaPlan) and accumulate_fused(g_ema, G, 0.999, plan) is plan
    assert rec.count('ema') == 2
    a, b = torch.nn.Linear(4, 3), torch.nn.Linear(4, 3)                              # CPU modules: the composite
    want = 0.25 * a.weight.detach() + 0.75 * b.weight.detach()
    with launches.observed() as rec:
        assert accumulate_fused(a, b, 0.25) is None
    assert rec.names == [] and torch.allclose(a.weight.detach(), want)


def test_ema_plan_declines(generators):
    from op.ema import EmaPlan
    G, _ = generators
    lin = lambda i, o: torch.nn.Linear(i, o).to(dev())      # noqa: E731
    assert 'shapes' in EmaPlan.declined(lin(4, 3), lin(5, 3))
    assert 'names' in EmaPlan.declined(lin(4, 3), torch.nn.Sequential(lin(4, 3)))
    assert 'float32' in EmaPlan.declined(lin(4, 3).half(), lin(4, 3))
    assert 'float32' in EmaPlan.declined(lin(4, 3), torch.nn.Linear(4, 3))            # a CPU parameter
    assert 'overlapping' in EmaPlan.declined(G, G)
    for pair in ((G, G), (lin(4, 3), lin(5, 3)), (lin(4, 3).half(), lin(4, 3))):
        with pytest.raises(RuntimeError, match='op.ema'):
            EmaPlan(*pair)


# ------------------------------------------------------------------------------------------------------- loss_row
ROWS = 3


def _loss_row_case(n, nulls, row):
    from op import _native
    store = torch.arange(1, 64, dtype=torch.float32, device=dev()) * 1.0009765625
    values = []
    for i in range(n):
        if i in nulls:
            values.append(None)
        elif i % 2:
            v = store[3 + 2 * i]                  # a 0-dim view at an odd element offset of a larger tensor
            assert v.ndim == 0 and (v.data_ptr() // 4) % 2 == 1
            values.append(v)
        else:
            values.append(torch.tensor(-0.5 - i, dtype=torch.float32, device=dev()))
    ring = torch.full((ROWS, 16), gpumem.SENTINEL, dtype=torch.float32, device=dev())
    with launches.observed() as rec:
        _native.loss_row(values, ring[row])
    torch.cuda.synchronize()
    assert rec.seen == [('loss_row', (n,))]
    want = torch.full((ROWS, 16), gpumem.SENTINEL, dtype=torch.float32)
    want[row] = torch.tensor([0.0 if (i >= n or values[i] is None) else values[i].item() for i in range(16)])
    assert torch.equal(ring.cpu(), want), (n, nulls, row)


@pytest.mark.parametrize('n,nulls,row', [(1, (), 0), (9, (), 1), (16, (), ROWS - 1), (9, (0,), 0), (9, (4,), ROWS - 1),
                                         (16, (15,), 1), (16, (0, 7, 15), 0), (1, (0,), 0), (0, (), 1)])
def test_loss_row(n, nulls, row):
    _loss_row_case(n, nulls, row)


def test_loss_row_refuses_17_values():
    from op import _native
    row = torch.zeros(16, dtype=torch.float32, device=dev())
    ptrs = (ctypes.c_void_p * 16)()
    assert lib().fmgan_loss_row_f32(ctypes.addressof(ptrs), 17, row.data_ptr(), None) == -1
    assert lib().fmgan_loss_row_f32(ctypes.addressof(ptrs), -1, row.data_ptr(), None) == -1
    assert lib().fmgan_loss_row_f32(None, 3, row.data_ptr(), None) == -1
    with launches.observed() as rec, pytest.raises(RuntimeError, match='loss_row'):
        _native.loss_row([None] * 17, row)
    assert rec.names == []
    with pytest.raises(RuntimeError):
        _native.loss_row([torch.zeros((), dtype=torch.float64, device=dev())], row)


# ------------------------------------------------------------------------------------------------------- train()
B = 2
FIELDS = (('D_Loss', 'd'), ('G_Loss', 'g'), ('G_Reg', 'g_reg'), ('L1_Loss', 'l1'), ('LPIPS_Loss', 'lpips'),
          ('Face_ID_Loss', 'face_id'), ('Heat_Map_Loss', 'hmap'), ('Face_Regional_Loss', 'face_reg'))


class FixedBatches:
    """A loader that assembles the training triple itself (as dataset.BankLoader does): fixed tensors, photos at 256^2
    for the encoders, render and target at the output's size."""

    def __init__(self, name, size):
        import ds_cases
        import synth
        self.photo = synth.tensor(f'{name}/photo', (B, 3, 256, 256), dist='uniform').to(dev())
        self.render = ds_cases.face_render(f'{name}/render', (B, 3, size, size)).to(dev())
        self.ref = synth.tensor(f'{name}/ref', (B, 3, size, size), dist='uniform').to(dev())
        self.asked = []

    def training_batch(self, pair=False, even_only=False):
        self.asked.append((pair, even_only))
        step = 2 if even_only else 1
        return self.photo[::step], self.render[::step], self.ref[::step]


def _lines(text):
    return [ln for ln in text.split('\n') if ln.startswith('Iter #: ')]


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    import test_checkpoint_gpu as CK
    import test_hip_train as H
    import train_3_encoder as T
    root = tmp_path_factory.mktemp('train_loop')
    args = H.train_args(ema_fuse=True, log_flush=3, iter=4, device=str(dev()))
    tr = T.Trainer(CK._nets(), args, dev())
    recorded = []
    step = tr.step

    def recording_step(*a, **k):
        ld = step(*a, **k)
        recorded.append({name: float(v.detach()) for name, v in ld.items()})
        return ld
    tr.step = recording_step
    loaders = tuple(FixedBatches(f'train_loop/{k}', CK.SIZE) for k in ('rec', 'ds', 'ep')) + (None,)
    log = io.StringIO()
    torch.manual_seed(11)
    np.random.seed(11)
    with launches.observed() as rec:
        ledger = T.train(args, loaders, (None, None), tr, None, str(root / 'exp'), log)
    fused = dict(names=list(rec.names), iter_idx=tr.iter_idx, log=log.getvalue(), flushes=ledger.flushes,
                 recorded=list(recorded), asked=[ld.asked[:] for ld in loaders[:3]], plan=tr.ema_plan)
    # one more iteration with the fused EMA switched off, on the same Trainer
    args.ema_fuse, args.iter = False, 5
    log2 = io.StringIO()
    with launches.observed() as rec:
        T.train(args, loaders, (None, None), tr, None, str(root / 'exp'), log2)
    return dict(fused=fused, unfused=dict(names=list(rec.names), iter_idx=tr.iter_idx, log=log2.getvalue()))


def test_train_on_the_smallest_trainer(trained):
    f = trained['fused']
    lines = _lines(f['log'])
    assert len(lines) == 4 and f['iter_idx'] == 4 and len(f['recorded']) == 4
    assert f['log'] == ''.join(ln + '\n' for ln in lines)
    flags = [(False, False), (True, False), (False, False), (True, False)]          # ds_freq 2, ex_ds_freq 3
    for i, (ln, rec, (ds, ex)) in enumerate(zip(lines, f['recorded'], flags)):
        print(ln, {name: rec.get(name) for _, name in FIELDS}, {k: rec[k] for k in ('ref_score', 'out_score') if k in rec})
        assert ln.startswith(f'Iter #: {i} Train Time: ')
        assert f' Dual Supervision: {ds} Extreme Pose DS: {ex} ' in ln
        assert float(re.search(r'Train Time: (\S+) ', ln).group(1)) >= 0.0
        for label, name in FIELDS:
            printed = re.search(f' {label}: (\\S+)', ln).group(1)
            assert printed == str(round(rec.get(name, 0.0), 3)), (i, label, printed, rec.get(name))
        # the comparison above is not one of zeros with zeros: the L1 distance to a uniform random target cannot be 0.
        # Nothing is asked of the other terms' values: with the suite's synthetic weights and learning rate the run
        # diverges at once (printed above: D's score of the generated image is -7730 before D's step of iteration 2 and
        # the G loss 4438 after it), and where that score comes out beyond +104 instead, float32 softplus(-x) is exactly
        # 0 and the line rightly says G_Loss: 0.0.
        assert rec['l1'] != 0.0
    assert f['recorded'][1]['face_reg'] != 0.0 and f['recorded'][0]['face_reg'] == 0.0
    assert f['asked'] == [[(False, False)] * 2, [(True, False)] * 2, []]
    assert f['names'].count('ema') == 4 and f['names'].count('loss_row') == 4
    assert f['flushes'] == 2 and f['plan'] is not None and f['plan'].rebuilds == 1
    u = trained['unfused']
    assert u['names'].count('ema') == 0 and u['names'].count('loss_row') == 1 and u['iter_idx'] == 5
    assert len(_lines(u['log'])) == 1 and u['log'].startswith('Iter #: 4 ')


# ------------------------------------------------------------------------------------------------------- main()
def test_main_from_a_folder_tree(tmp_path, monkeypatch):
    """main(argv) with the folders of dataset_cases.write_tree on its command line.  The tree's images are 12^2 and 24^2,
    resized to --size 64 by Dataset_DataLoader_Setup as it stands, and the tensor encoder needs 256^2 photos (its 4 x 4
    output feeds the Generator's first layer): the tree cannot feed a training iteration.  So the data path is left as it
    is and this test stands its own loaders in for Dataset_DataLoader_Setup's (fixed batches, photos at 256^2), as
    tests/test_checkpoint_gpu.py feeds its Trainer; everything else is main()'s: the arguments, Module_To_Train_Setup (with
    D_edit), the Trainer, the experiment folder, the log and the loop.  No visual samples (--visual_real_img_dir unset)."""
    import dataset_cases
    import train_3_encoder as T
    dirs = dataset_cases.write_tree(tmp_path / 'tree')
    asked = {}

    def loaders(args, device=None, resident=True):
        asked.update(size=args.size, rec_batch=args.rec_batch, synface_dir=args.synface_dir, resident=resident)
        rec, ds, ep = (FixedBatches(f'main/{k}', args.size) for k in ('rec', 'ds', 'ep'))
        return None, None, None, rec, ds, ep, None, None, None
    monkeypatch.setattr(T, 'Dataset_DataLoader_Setup', loaders)
    exp_dir = str(tmp_path / 'exp')
    torch.manual_seed(3)
    np.random.seed(3)
    out = T.main(['--size', '64', '--n_mlp', '2', '--rec_batch', '2', '--ds_batch', '2', '--iter', '2', '--use_loss_nets',
                  'false', '--exp_dir', exp_dir, '--synface_dir', dirs['synface'], '--extreme_pose_dir', dirs['synface'],
                  '--ffhq_train_img_dir', os.path.dirname(dirs['img']), '--tsr_encode', 'Photo Image', '--device',
                  str(dev())])
    assert out == exp_dir and asked == dict(size=64, rec_batch=2, synface_dir=dirs['synface'], resident=True)
    logs = [f for f in os.listdir(exp_dir) if f.endswith('_training_log.out')]
    assert len(logs) == 1 and os.path.isdir(os.path.join(exp_dir, 'sample')) and os.path.isdir(os.path.join(exp_dir, 'ckpt'))
    text = open(os.path.join(exp_dir, logs[0])).read()
    assert text.startswith('\n--------------- Training Start ---------------\n\nParams: \n\n  Model and Training Data: \n'
                           f'    Synthetic Data Folder: {dirs["synface"]}\n')
    for piece in ('    Generator Num Layers: 10\n', '    Generated Image Size: 64\n', '    Using Separate Discriminator: True\n',
                  '    Training Iterations: 2\n', '    Number of GPUs: 1\n', '    Heat Map Loss Iteration Threshold: inf\n'):
        assert piece in text, piece
    lines = _lines(text)
    assert len(lines) == 2 and ' Dual Supervision: False ' in lines[0] and ' Dual Supervision: True ' in lines[1]
    assert text.index('Visual Real Samples Directory: None\n\n') < text.index(lines[0])
    assert re.search(r'\n\nTotal training time: \d+\.\d+$', text)
