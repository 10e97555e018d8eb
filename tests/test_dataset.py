"""The data side on the CPU (dataset.py, op/image_bank.py, train_3_encoder.Dataset_DataLoader_Setup): the samplers' index
sequences and the dataset classes' file lists and items against those recorded from the reference
(tests/golden/dataset.npz, tools/make_golden_dataset.py), BankLoader against torch's BatchSampler and DataLoader, the
training triples against Data_Loading over plain batches, bank persistence, and the host-side checks.  Banks on a CPU
device take bank_gather's composite form, so everything but the kernel is exercised here."""
import os

import numpy as np
import pytest
import torch
from torch.utils import data

import dataset_cases as C
import launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seeded_sampler(cls, n):
    np_seed, torch_seed = C.SAMPLER_SEED[n]
    np.random.seed(np_seed)
    gen = torch.Generator()
    gen.manual_seed(torch_seed)
    return cls(C.Sized(n), C.N_IMG_PER_ID, generator=gen)


# ------------------------------------------------------------------------------------------------ samplers
@pytest.mark.parametrize('n', C.SAMPLER_LENS)
def test_dual_supervision_sampler_yields_the_reference_sequence(golden, n):
    import dataset
    g = golden('dataset')
    s = _seeded_sampler(dataset.DualSupervisionSampler, n)
    seq = list(s)
    assert seq == g[f'sampler/dual/{n}'].tolist()
    assert len(s) == int(g[f'sampler/dual/{n}/len']) == 2 * n == len(seq)
    assert sorted(seq[0::2]) == list(range(n))                           # a permutation, each followed by its partner
    for a, b in zip(seq[0::2], seq[1::2]):
        assert a // C.N_IMG_PER_ID == b // C.N_IMG_PER_ID and a != b


@pytest.mark.parametrize('n', C.SAMPLER_LENS)
def test_extreme_pose_sampler_yields_the_reference_sequence(golden, n):
    import dataset
    g = golden('dataset')
    s = _seeded_sampler(dataset.ExtremePoseDualSupervisionSampler, n)
    seq = list(s)
    assert seq == g[f'sampler/extreme/{n}'].tolist()
    assert len(s) == int(g[f'sampler/extreme/{n}/len']) == 2 * n // C.N_IMG_PER_ID == len(seq)
    assert sorted(seq[0::2]) == [C.N_IMG_PER_ID * p for p in range(n // C.N_IMG_PER_ID)]
    for a, b in zip(seq[0::2], seq[1::2]):
        assert a % C.N_IMG_PER_ID == 0 and a // C.N_IMG_PER_ID == b // C.N_IMG_PER_ID and a != b


def test_sampler_constructor_checks_and_lengths():
    import dataset
    for cls in (dataset.DualSupervisionSampler, dataset.ExtremePoseDualSupervisionSampler):
        with pytest.raises(TypeError):
            cls(C.Sized(21), 7, replacement=1)
        with pytest.raises(ValueError):
            cls(C.Sized(21), 7, num_samples=5)
        with pytest.raises(ValueError):
            cls(C.Sized(0), 7)
        assert len(cls(C.Sized(21), 7, replacement=True, num_samples=5)) == 5
    assert len(dataset.ExtremePoseDualSupervisionSampler(C.Sized(25), 7)) == 50 // 7      # 2 * len // n, not 2 * (len // n)
    assert dataset.Swap_List_Pair(range(4)) == [1, 0, 3, 2]


# ------------------------------------------------------------------------------------------------ file lists, items
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    pytest.importorskip('PIL.Image')
    root = tmp_path_factory.mktemp('dataset_tree')
    return root, C.write_tree(root)


def test_file_lists_and_items_equal_the_recorded_ones(golden, tree):
    import dataset
    g = golden('dataset')
    root, dirs = tree
    sets = C.build_datasets(dataset, dirs)
    for name, ds in sets.items():
        assert len(ds) == int(g[f'files/{name}/len']), name
        for key, paths in C.file_lists(ds).items():
            got = C.relative(paths, root) if key != 'ids' else list(paths)
            assert got == g[f'files/{name}/{key}'].tolist(), (name, key)
        if name == 'editing_train':
            np.random.seed(C.EDIT_TRAIN_SEED)
        for i in range(len(ds)):
            arrays = C.item_arrays(ds[i])
            assert len(arrays) == {'ffhq': 1, 'editing': 5, 'editing_train': 3}.get(name, 2)
            for k, a in enumerate(arrays):
                want = g[f'items/{name}/{i}/{k}']
                assert a.dtype == np.uint8 and a.shape == want.shape and np.array_equal(a, want), (name, i, k)
    syn = sets['synthetic']
    assert syn.id_list == ['id_1', 'id_10', 'id_2'] and len(syn) == 21
    assert not any('contact_sheet' in p for p in syn.g_img_list + syn.r_img_list)


def test_transform_is_resize_totensor_normalize(tree):
    """Transform against its definition, written out with PIL and numpy: the bilinear resize to Resize(size)'s output
    size (shorter edge -> size), then ((x / 255) - mean) / std in float32."""
    from PIL import Image
    import dataset
    _, dirs = tree
    ds = dataset.FFHQ_Dataset(dirs['img'])
    img = ds[1]
    big = Image.fromarray(C.image('transform/wide', 10, 30))
    for im, (oh, ow) in ((img, (C.SIZE, C.SIZE)), (big, (8, 24))):
        t = dataset.Transform(C.SIZE, mean=0.25, std=0.5)(im)
        ref = np.asarray(im.resize((ow, oh), Image.BILINEAR)).astype(np.float32).transpose(2, 0, 1)
        ref = ((ref / np.float32(255)) - np.float32(0.25)) / np.float32(0.5)
        assert t.dtype == torch.float32 and tuple(t.shape) == (3, oh, ow) and t.is_contiguous()
        assert np.array_equal(t.numpy(), ref)
    same = dataset.Transform(10)(Image.fromarray(C.image('transform/same', 10, 30)))        # shorter edge == size: untouched
    assert tuple(same.shape) == (3, 10, 30)


# ------------------------------------------------------------------------------------------------ loaders
def _resident_and_dataset(name, dirs):
    import dataset
    ds = C.build_datasets(dataset, dirs, dataset.Transform(C.SIZE))[name]
    return dataset.Resident(ds, C.SIZE, 'cpu'), ds


@pytest.fixture(scope='module')
def residents(tree):
    _, dirs = tree
    return {name: _resident_and_dataset(name, dirs) for name in ('ffhq', 'synthetic', 'reconstruction', 'editing',
                                                                 'editing_train')}


def _samplers(kind, source, seed):
    import dataset
    gen = torch.Generator()
    gen.manual_seed(seed)
    if kind == 'sequential':
        return data.SequentialSampler(source)
    if kind == 'random':
        return data.RandomSampler(source, generator=gen)
    cls = dataset.DualSupervisionSampler if kind == 'dual' else dataset.ExtremePoseDualSupervisionSampler
    return cls(source, C.N_IMG_PER_ID, generator=gen)


@pytest.mark.parametrize('drop_last', [False, True])
@pytest.mark.parametrize('kind', ['sequential', 'random', 'dual', 'extreme'])
def test_bank_loader_batches_are_batch_samplers(residents, kind, drop_last):
    import dataset
    res, _ = residents['synthetic']
    for batch_size in (4, 5):
        np.random.seed(3)
        want = list(data.BatchSampler(_samplers(kind, res, 9), batch_size, drop_last))
        np.random.seed(3)
        loader = dataset.BankLoader(res, batch_size, _samplers(kind, res, 9), drop_last)
        got = []
        for batch in loader:
            got.append(list(loader.indices))
            assert batch[0].shape[0] == len(loader.indices)
        assert got == want and len(loader) == len(want)


def _assert_batches_equal(a, b):
    a = list(a) if isinstance(a, (list, tuple)) else [a]
    b = list(b) if isinstance(b, (list, tuple)) else [b]
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == torch.float32 and torch.equal(x, y)


@pytest.mark.parametrize('name', ['ffhq', 'synthetic', 'reconstruction', 'editing', 'editing_train'])
def test_bank_loader_equals_a_dataloader(residents, name):
    """Two epochs: the same batches, bit for bit, as DataLoader(dataset with Transform, num_workers=0) over the same
    sampler — for train=True editing data with the same np.random.choice draws, so the same edit renders."""
    import dataset
    res, ds = residents[name]
    assert len(res) == len(ds) and len(res.banks) == {'ffhq': 1, 'editing_train': 3}.get(name, 2)
    kind = 'dual' if name == 'synthetic' else 'random'
    for batch_size, drop_last in ((4, False), (4, True)):
        np.random.seed(8)
        ref = data.DataLoader(ds, batch_size=batch_size, sampler=_samplers(kind, ds, 4), num_workers=0,
                              drop_last=drop_last)
        want = [b for _ in range(2) for b in ref]
        np.random.seed(8)
        loader = dataset.BankLoader(res, batch_size, _samplers(kind, res, 4), drop_last)
        got = [b for _ in range(2) for b in loader]
        assert len(got) == len(want) == 2 * len(loader)
        for a, b in zip(got, want):
            _assert_batches_equal(a, b)
    # an item of the Resident is the dataset's item
    np.random.seed(2)
    a = res[len(res) - 1]
    np.random.seed(2)
    _assert_batches_equal(a, ds[len(ds) - 1])


def _plain_stream(res, batch_size, kind, seed):
    """(photo, render) batches as tuples from a generator: a loader WITHOUT training_batch, today's Data_Loading path."""
    import dataset
    loader = dataset.BankLoader(res, batch_size, _samplers(kind, res, seed))
    while True:
        for batch in loader:
            yield batch


def test_training_triples_equal_data_loading_over_plain_batches(residents):
    import dataset
    import train_3_encoder as T
    res, _ = residents['synthetic']
    cpu = torch.device('cpu')
    flags = [(False, False), (True, False), (True, True)] * 4           # runs past the epoch's end of every loader

    def run(fused):
        np.random.seed(5)
        if fused:
            mk = lambda bs, kind, seed: T.sample_data(dataset.BankLoader(res, bs, _samplers(kind, res, seed)))
        else:
            mk = lambda bs, kind, seed: _plain_stream(res, bs, kind, seed)
        rec, ds_, ep = mk(5, 'random', 1), mk(6, 'dual', 2), mk(4, 'extreme', 3)
        assert hasattr(rec, 'training_batch') == fused
        return [dataset.Data_Loading(rec, ds_, f, cpu, extreme_loader=ep, extreme_ds_flag=e) for f, e in flags]

    with launches.observed() as rec:
        fused = run(True)
    assert rec.seen == []                                               # CPU banks: the composite, no launch bracket
    plain = run(False)
    for (f, e), a, b in zip(flags, fused, plain):
        assert len(a) == len(b) == 3
        for x, y in zip(a, b):
            assert torch.equal(x, y) and x.dtype == torch.float32
        g_input, r_input, g_ref = a
        # extreme pose: 6 entries per epoch in batches of 4 and 2, halved; reconstruction: 21 in fives, the last one alone
        assert g_input.shape[0] in ((2, 1) if e else ((6,) if f else (5, 1)))
        if not f:
            assert torch.equal(g_ref, g_input) and g_ref.data_ptr() != g_input.data_ptr()
        # the three tensors are contiguous views of one allocation
        assert all(t.is_contiguous() for t in a)
        assert g_input.untyped_storage().data_ptr() == r_input.untyped_storage().data_ptr() == \
            g_ref.untyped_storage().data_ptr()


def test_data_loading_ffhq_branch(residents):
    import dataset
    import train_3_encoder as T
    edit, _ = residents['editing_train']
    pure, _ = residents['ffhq']
    np.random.seed(4)
    ds_loader = T.sample_data(dataset.BankLoader(edit, 3, data.SequentialSampler(edit)))
    pure_loader = T.sample_data(dataset.BankLoader(pure, 3, data.SequentialSampler(pure)))
    out = dataset.Data_Loading(None, ds_loader, True, torch.device('cpu'), pure_ffhq_loader=pure_loader,
                               ds_dataset_type='FFHQ')
    assert len(out) == 5 and all(tuple(t.shape) == (3, 3, C.SIZE, C.SIZE) for t in out)
    g_input, r_input, r_edit, g_ref, ffhq_ref = out
    np.random.seed(4)
    items = [edit[i] for i in range(3)]
    for k, t in enumerate((g_input, r_input, r_edit)):
        assert torch.equal(t, torch.stack([it[k] for it in items]))
    assert torch.equal(g_ref, g_input) and g_ref.data_ptr() != g_input.data_ptr()
    assert torch.equal(ffhq_ref, torch.stack([pure[i] for i in range(3)]))
    with pytest.raises(ValueError):
        dataset.Data_Loading(None, ds_loader, True, 'cpu', ds_dataset_type='Other')


def test_setup_drives_loaders_from_a_folder_tree(tree, tmp_path):
    """Dataset_DataLoader_Setup over the tree: the 9-tuple, training triples of the reference's batch sizes from the
    resident loaders, the same shapes from the non-resident ones, and the banks kept in bank_cache_dir."""
    import dataset
    import train_3_encoder as T
    root, dirs = tree
    ffhq = os.path.dirname(dirs['img'])
    args = T.default_args(size=C.SIZE, synface_dir=dirs['synface'], extreme_pose_dir=dirs['synface'],
                          ffhq_train_img_dir=ffhq, quant_eval_img_dir=ffhq, rec_batch=4, ds_batch=4,
                          quant_eval_batch_size=8, num_workers=0, bank_cache_dir=str(tmp_path / 'banks'))
    assert T.default_args().num_workers == 8 and T.default_args().bank_cache_dir is None
    for resident in (True, False):
        out = T.Dataset_DataLoader_Setup(args, device='cpu', resident=resident)
        assert len(out) == 9
        transform, syn, ep, rec_l, ds_l, ep_l, pure_l, rec_eval, edit_eval = out
        assert isinstance(transform, dataset.Transform) and len(syn) == len(ep) == 21
        assert isinstance(syn, dataset.Resident if resident else dataset.Synthetic_Dataset)
        assert hasattr(rec_l, 'training_batch') == resident
        cpu = torch.device('cpu')
        # the extreme-pose batch: 2 * ds_batch = 8 positions, of which the 3 identities fill 6; their even members
        for flags, n in (((False, False), 4), ((True, False), 4), ((True, True), 3)):
            triple = dataset.Data_Loading(rec_l, ds_l, flags[0], cpu, extreme_loader=ep_l, extreme_ds_flag=flags[1])
            assert [tuple(t.shape) for t in triple] == [(n, 3, C.SIZE, C.SIZE)] * 3
        assert tuple(next(pure_l).shape) == (2, 3, C.SIZE, C.SIZE)
        rec_batches, edit_batches = list(rec_eval), list(edit_eval)
        assert [b[0].shape[0] for b in rec_batches] == [6] and [len(b) for b in edit_batches] == [5] * 3
        g, r = syn[3]
        assert tuple(g.shape) == tuple(r.shape) == (3, C.SIZE, C.SIZE)
    kept = sorted(os.listdir(tmp_path / 'banks'))
    assert f'synface_{C.SIZE}.0.npy' in kept and f'synface_{C.SIZE}.1.npy' in kept
    again = T.Dataset_DataLoader_Setup(args, device='cpu')[1]             # read back from the cache
    assert torch.equal(again.banks[0].data, dataset.Resident(dataset.Synthetic_Dataset(dirs['synface']), C.SIZE,
                                                               'cpu').banks[0].data)
    with pytest.raises(ValueError):
        T.Dataset_DataLoader_Setup(T.default_args(synface_dir=dirs['synface'], extreme_pose_dir=dirs['synface']), 'cpu')


def test_train_iteration_draws_its_batches_from_the_setup(tree):
    """Trainer.train_iteration's schedule over Dataset_DataLoader_Setup's loaders, with the step itself recorded instead of
    run (the networks have no CPU path): six iterations are rec, ds, rec, ds, rec, extreme, each with the triple its
    loader assembles — the pairs of a dual-supervision batch share an identity, the extreme batch is half its positions."""
    import dataset
    import train_3_encoder as T
    _, dirs = tree
    args = T.default_args(size=C.SIZE, synface_dir=dirs['synface'], extreme_pose_dir=dirs['synface'],
                          rec_dataset_type='Synthetic', rec_batch=4, ds_batch=4)
    _, syn, _, rec_l, ds_l, ep_l, pure_l, rec_eval, edit_eval = T.Dataset_DataLoader_Setup(args, device='cpu')
    assert pure_l is None and rec_eval is None and edit_eval is None          # no FFHQ folders given
    tr = T.Trainer.__new__(T.Trainer)
    tr.args, tr.device, tr.iter_idx, tr.ds_count, seen = args, torch.device('cpu'), 0, 0, []

    def step(g_input, r_input, g_ref, ppl_choice=None, ds_flag=False, extreme_ds_flag=False):
        seen.append((g_input, r_input, g_ref, list(ds_l.loader.indices or []), list(ep_l.loader.indices or [])))
        tr.iter_idx += 1
        return {}
    tr.step = step
    flags = [tr.train_iteration(rec_l, ds_l, ep_l)[1:] for _ in range(6)]
    assert flags == [(False, False), (True, False), (False, False), (True, False), (False, False), (True, True)]
    assert [s[0].shape[0] for s in seen] == [4, 4, 4, 4, 4, 3]
    photo = lambda i: syn[i][0]
    render = lambda i: syn[i][1]
    g_input, r_input, g_ref, ds_idx, _ = seen[1]
    for b, i in enumerate(ds_idx):
        partner = ds_idx[b ^ 1]
        assert partner // 7 == i // 7 and partner != i
        assert torch.equal(g_input[b], photo(i)) and torch.equal(r_input[b], render(partner))
        assert torch.equal(g_ref[b], photo(partner))
    g_input, r_input, g_ref, _, ep_idx = seen[5]
    assert len(ep_idx) == 6
    for m in range(3):
        assert ep_idx[2 * m] % 7 == 0
        assert torch.equal(g_input[m], photo(ep_idx[2 * m])) and torch.equal(r_input[m], render(ep_idx[2 * m + 1]))
        assert torch.equal(g_ref[m], photo(ep_idx[2 * m + 1]))


# ------------------------------------------------------------------------------------------------ banks
def test_image_bank_round_trip_and_constructors(tmp_path):
    from op.image_bank import ImageBank
    a = C.image('bank/a', 10 * 6, 5).reshape(10, 6, 5, 3)
    bank = ImageBank.from_arrays(a)
    assert len(bank) == 10 and bank.size == (6, 5) and bank.device.type == 'cpu'
    assert torch.equal(ImageBank.from_arrays(list(a)).data, bank.data)
    assert torch.equal(ImageBank.from_arrays([torch.from_numpy(x) for x in a]).data, bank.data)
    path = tmp_path / 'bank.npy'
    bank.save(path)
    assert np.array_equal(np.load(path), a)                              # a plain .npy
    back = ImageBank.load(path, 'cpu')
    assert back.data.dtype == torch.uint8 and torch.equal(back.data, bank.data)
    with pytest.raises(ValueError):
        ImageBank.from_arrays([a[0], a[1][:3]])
    with pytest.raises(ValueError):
        ImageBank.from_arrays(a.astype(np.float32))


def test_image_bank_from_files(tree):
    """Equal sources, unequal sources (the host resize) and sources that stay unequal; at most 16 decode threads."""
    from PIL import Image
    import dataset
    from op import image_bank
    from op.image_bank import ImageBank
    _, dirs = tree
    paths = dataset.FFHQ_Dataset(dirs['img']).images_list
    bank = ImageBank.from_files(paths, C.SIZE, 'cpu', chunk=4, workers=64)
    assert image_bank.MAX_WORKERS == 16 and tuple(bank.data.shape) == (len(paths), C.SIZE, C.SIZE, 3)
    for i, p in enumerate(paths):
        im = Image.open(p).convert('RGB')
        want = np.asarray(im.resize((C.SIZE, C.SIZE), Image.BILINEAR)) if im.size != (C.SIZE, C.SIZE) else np.asarray(im)
        assert np.array_equal(bank.data[i].numpy(), want)
    wide = os.path.join(os.path.dirname(dirs['img']), 'wide.png')
    Image.fromarray(C.image('files/wide', 12, 20)).save(wide)
    try:
        with pytest.raises(ValueError):
            ImageBank.from_files(paths[:2] + [wide], C.SIZE, 'cpu')
    finally:
        os.remove(wide)


# ------------------------------------------------------------------------------------------------ host-side checks
def test_validation_errors_come_before_any_launch():
    from op import image_bank
    from op.image_bank import EpochIndex, ImageBank
    a = ImageBank.from_arrays(C.image('check/a', 6 * 4, 4).reshape(6, 4, 4, 3))
    b = ImageBank.from_arrays(C.image('check/b', 6 * 4, 4).reshape(6, 4, 4, 3))
    small = ImageBank.from_arrays(C.image('check/s', 3 * 4, 4).reshape(3, 4, 4, 3))
    other = ImageBank.from_arrays(C.image('check/o', 6 * 4, 5).reshape(6, 4, 5, 3))
    index = EpochIndex([0, 5, 2, 3, 1], 6, 'cpu', partner=[0, 1, 2, 0, 1], partner_limit=3)
    pair = [(0, 0), (1, 1)]
    with launches.observed() as rec:
        for bad in ([0, 6], [-1, 2]):
            with pytest.raises(IndexError):
                EpochIndex(bad, 6, 'cpu')                                           # range, at upload time
        with pytest.raises(IndexError):
            EpochIndex([0, 1], 6, 'cpu', partner=[0, 3], partner_limit=3)
        with pytest.raises(IndexError):
            EpochIndex([0, 1], 6, 'cpu', partner=[0], partner_limit=3)
        with pytest.raises(ValueError):
            image_bank.bank_gather([a, other], index, 0, 4, pair)                   # unequal H x W
        with pytest.raises(ValueError):
            image_bank.bank_gather([a.data.float()], index, 0, 4, [(0, 0)])         # dtype
        with pytest.raises(ValueError):
            image_bank.bank_gather([a.data[:, :, ::2]], index, 0, 4, [(0, 0)])      # not contiguous
        with pytest.raises(RuntimeError):
            image_bank.bank_gather([a, b.data.to('meta')], index, 0, 4, pair)       # another device
        with pytest.raises(IndexError):
            image_bank.bank_gather([a, b], index, 0, 5, pair)                       # odd batch with a swap
        with pytest.raises(IndexError):
            image_bank.bank_gather([a, b], index, 0, 3, [(0, 0)], even_only=True)
        with pytest.raises(IndexError):
            image_bank.bank_gather([a, b], index, 2, 4, [(0, 0)])                   # past the end of the epoch's list
        with pytest.raises(IndexError):
            image_bank.bank_gather([a, small], index, 0, 4, pair)                   # the list can leave a smaller bank
        with pytest.raises(IndexError):
            image_bank.bank_gather([a, b], index, 0, 4, [(0, 0, 0, 4, 1)])          # index * 4 + 1 leaves the bank
        with pytest.raises(ValueError):
            image_bank.bank_gather([a, b], index, 0, 4, [(2, 0)])                   # no such bank
        with pytest.raises(ValueError):
            image_bank.bank_gather([a, b], EpochIndex([0, 1], 6, 'cpu'), 0, 2, [(0, 0, 1, 1, 0)])   # no partner list
        with pytest.raises(ValueError):
            image_bank.bank_gather([a, b], index, 0, 4, pair, out=torch.empty(7, 3, 4, 4))
        with pytest.raises(ValueError):
            image_bank.bank_gather([a, b], index, 0, 4, pair, std=0.0)
        with pytest.raises(ValueError):
            image_bank.bank_gather([a] * 5, index, 0, 4, [(0, 0)])
        out = image_bank.bank_gather([a, small], index, 1, 4, [(0, 1), (1, 0, 1, 1, 0)], mean=0.25)
    assert rec.seen == []
    want_a = a.data[[2, 5, 1, 3]].permute(0, 3, 1, 2).float().div(255).sub(0.25).div(0.5)
    want_s = small.data[[1, 2, 0, 1]].permute(0, 3, 1, 2).float().div(255).sub(0.25).div(0.5)
    assert torch.equal(out[:4], want_a) and torch.equal(out[4:], want_s)


def test_bank_fuse_switch_follows_the_convention():
    """FMGAN_NO_BANK_FUSE=1 is read at import, as the other FMGAN_NO_*_FUSE switches are, into image_bank.BANK_FUSE."""
    import subprocess
    import sys
    code = ('import sys; sys.path[:0] = [%r, %r]; from op import image_bank; print(image_bank.BANK_FUSE)'
            % (ROOT, os.path.join(ROOT, '3d-fm-gan_amd')))
    for value, want in ((None, 'True'), ('1', 'False'), ('0', 'True')):
        env = {k: v for k, v in os.environ.items() if k != 'FMGAN_NO_BANK_FUSE'}
        if value is not None:
            env['FMGAN_NO_BANK_FUSE'] = value
        assert subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                              check=True).stdout.strip() == want


def test_library_refuses_bad_gather_arguments_without_a_launch():
    """fmgan_bank_gather's argument checks return before any HIP call (the pointers are placeholders)."""
    import ctypes
    from nets import lib
    L = lib()
    fake = ctypes.c_void_p(0x1000)
    groups = (ctypes.c_int * 10)(0, 0, 0, 1, 0, 1, 0, 1, 1, 0)

    def call(h=8, w=8, members=4, stride=1, n_groups=2, std=0.5, pix=0, offset=0, out=fake, index=fake, count0=6,
             table=groups):
        return L.fmgan_bank_gather(fake, fake, None, None, count0, 6, 0, 0, h, w, index, 8, None, 0, offset, members, stride,
                                   table, n_groups, out, 0.5, std, pix, None)
    assert call(members=0) == 0                                           # empty: nothing to do
    for kw in (dict(h=0), dict(w=-1), dict(members=-1), dict(stride=3), dict(stride=0), dict(n_groups=0),
               dict(n_groups=9), dict(std=0.0), dict(pix=8), dict(offset=-1), dict(out=None), dict(index=None),
               dict(count0=-1), dict(table=None), dict(table=(ctypes.c_int * 10)(0, 0, 2, 1, 0, 1, 0, 1, 1, 0))):
        assert call(**kw) == -1, kw
    assert call(h=1 << 15, w=1 << 15) == -4                               # pixel indices are 32-bit


def test_bank_gather_kernels_fit_the_streaming_budget(tmp_path):
    """No scratch, no spills and at most 64 VGPRs (8 waves per SIMD) for each instantiation of the new kernel: the budget
    tests/test_kernel_budgets.py holds the other streaming kernels to."""
    import codeobj
    notes = codeobj.kernel_notes(tmp_path)
    names = [k for k in notes if 'bank_gather' in k]
    assert len(names) == 3, names                                          # P = 4, P = 16, scalar
    for n in names:
        k = notes[n]
        assert k['vgpr'] <= 64 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0, (n, k)
