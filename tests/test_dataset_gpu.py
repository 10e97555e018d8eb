"""fmgan_bank_gather on the GPU (csrc/image_bank.hip through op/image_bank.py and dataset.BankLoader): every comparison
is torch.equal against the composite over CPU banks (index_select + ((x / 255) - mean) / std in torch), every output sits
between gpumem.guarded sentinels, and the launch brackets are counted."""
import numpy as np
import pytest
import torch

import dataset_cases as C
import gpumem
import launches

pytestmark = pytest.mark.gpu


def _images(tag, n, h, w):
    return C.image(tag, n * h, w).reshape(n, h, w, 3)


def _banks(arrays, device):
    from op.image_bank import ImageBank
    return [ImageBank.from_arrays(a, device) for a in arrays]


def _index(order, limit, device, partner=None, partner_limit=None):
    from op.image_bank import EpochIndex
    return EpochIndex(order, limit, device, partner=partner, partner_limit=partner_limit)


def _check(arrays, order, offset, batch, groups, even_only=False, mean=0.5, std=0.5, partner=None, partner_limit=None,
           gpu_banks=None, misaligned_out=False, brackets=1):
    """bank_gather on GPU banks into a guarded buffer against the same call on CPU banks; returns the GPU result."""
    from op import image_bank
    limit = len(arrays[0])
    want = image_bank.bank_gather(_banks(arrays, 'cpu'), _index(order, limit, 'cpu', partner, partner_limit), offset, batch,
                                  groups, even_only=even_only, mean=mean, std=std)
    gpu_banks = gpu_banks if gpu_banks is not None else _banks(arrays, gpumem.dev())
    index = _index(order, limit, gpumem.dev(), partner, partner_limit)
    if misaligned_out:
        n = want.numel()
        buf = torch.full((n + 2 * gpumem.GUARD + 1,), float('nan'), dtype=torch.float32, device=gpumem.dev())
        buf[:gpumem.GUARD + 1] = gpumem.SENTINEL
        buf[gpumem.GUARD + 1 + n:] = gpumem.SENTINEL
        view = buf[gpumem.GUARD + 1:gpumem.GUARD + 1 + n].view(want.shape)
        assert view.data_ptr() % 16 == 4
        intact = lambda: bool((buf[:gpumem.GUARD + 1] == gpumem.SENTINEL).all()) and \
            bool((buf[gpumem.GUARD + 1 + n:] == gpumem.SENTINEL).all())
    else:
        buf, view = gpumem.guarded(tuple(want.shape))
        intact = lambda: gpumem.guards_intact(buf)
    with launches.observed() as rec:
        got = image_bank.bank_gather(gpu_banks, index, offset, batch, groups, even_only=even_only, mean=mean, std=std,
                                     out=view)
    assert got.data_ptr() == view.data_ptr() and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    assert intact()
    assert rec.names == ['bank_gather'] * brackets
    return got


REC = [(0, 0), (1, 0), (0, 0)]          # (g_input, r_input, g_ref) of a reconstruction batch
PAIR = [(0, 0), (1, 1), (0, 1)]         # ... of a dual-supervision batch: the partner's render and photo


@pytest.mark.parametrize('mode', ['reconstruction', 'pair', 'pair_even'])
def test_pairing_modes(mode):
    arrays = [_images('gpu/pair/a', 6, 8, 8), _images('gpu/pair/b', 6, 8, 8)]
    order = [4, 1, 5, 0, 2, 3, 3, 1]
    groups = REC if mode == 'reconstruction' else PAIR
    for offset in (0, 4, 2):                                   # one bracket per batch
        got = _check(arrays, order, offset, 4, groups, even_only=mode == 'pair_even')
        assert got.shape[0] == 3 * (2 if mode == 'pair_even' else 4)
    if mode == 'pair':                                         # spelled out once: member b reads the image of b ^ 1
        got = _check(arrays, order, 0, 4, PAIR)
        ref = torch.from_numpy(arrays[1][[1, 4, 0, 5]]).permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)
        assert torch.equal(got[4:8].cpu(), ref)


@pytest.mark.parametrize('h,w', [(5, 7), (6, 6), (1, 1), (1, 3), (8, 8), (4, 4)])
def test_small_and_odd_shapes(h, w):
    """5 x 7: H*W odd; 6 x 6: H*W % 4 == 0 with W % 4 != 0; 1 x 1 and 1 x 3; 8 x 8 and 4 x 4: the two vector widths' smallest
    images, two images so that the second starts at an image stride."""
    arrays = [_images(f'gpu/shape/{h}x{w}/a', 5, h, w), _images(f'gpu/shape/{h}x{w}/b', 5, h, w)]
    _check(arrays, [3, 0, 4, 4, 1, 2], 1, 4, PAIR)
    _check(arrays, [3, 0, 4, 4, 1, 2], 0, 5, [(1, 0)])


@pytest.mark.parametrize('h,w', [(8, 8), (5, 7)])
def test_bank_view_one_byte_into_its_storage(h, w):
    from op.image_bank import ImageBank
    a = _images(f'gpu/offset/{h}x{w}', 4, h, w)
    store = torch.zeros(a.size + 1, dtype=torch.uint8, device=gpumem.dev())
    view = store[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 4 == 1
    _check([a], [2, 3, 0, 1], 0, 4, [(0, 1)], gpu_banks=[ImageBank(view)])


@pytest.mark.parametrize('h,w', [(8, 8), (6, 6), (5, 7)])
def test_misaligned_output(h, w):
    _check([_images(f'gpu/misout/{h}x{w}', 4, h, w)], [2, 3, 0, 1], 0, 4, [(0, 0), (0, 1)], misaligned_out=True)


@pytest.fixture(scope='module')
def real_arrays():
    return [_images('gpu/real/a', 21, 256, 256), _images('gpu/real/b', 21, 256, 256)]


def test_real_shape_with_duplicates(real_arrays):
    order = [20, 3, 3, 7, 0, 20, 11, 11, 5, 6, 7, 8, 19, 19, 19, 2] + [13] * 16
    _check(real_arrays, order, 0, 16, PAIR)                    # duplicate indices in one batch
    _check(real_arrays, order, 16, 16, REC)                    # a batch of one repeated index
    _check(real_arrays, order, 8, 16, PAIR, even_only=True)


@pytest.mark.parametrize('pix', [4, 16])
@pytest.mark.parametrize('h,w', [(256, 256), (8, 8), (4, 5)])
def test_both_vector_widths(real_arrays, pix, h, w):
    """The raw entry with pixels_per_lane forced: both instantiations of the vector kernel give the composite's bits
    (4 x 5: H*W % 16 != 0, where a request for 16 is served at 4)."""
    from op import _native, image_bank
    arrays = real_arrays if h == 256 else [_images(f'gpu/width/{h}x{w}/a', 21, h, w), _images(f'gpu/width/{h}x{w}/b', 21, h, w)]
    order = [5, 20, 0, 9, 9, 1, 17, 3]
    groups = [(0, 0, 0, 1, 0), (1, 0, 1, 1, 0), (0, 0, 1, 1, 0)]          # (bank, source, swap, mul, add): the PAIR triple
    want = image_bank.bank_gather(_banks(arrays, 'cpu'), _index(order, 21, 'cpu'), 0, 8, PAIR)
    gpu = [b.data for b in _banks(arrays, gpumem.dev())]
    buf, view = gpumem.guarded(tuple(want.shape))
    with launches.observed() as rec:
        got = _native.bank_gather(gpu, _index(order, 21, gpumem.dev()).data, None, 0, 8, 1, groups, out=view,
                                  pixels_per_lane=pix)
    assert torch.equal(got.cpu(), want) and gpumem.guards_intact(buf)
    assert rec.seen == [('bank_gather', (24, h, w, 3, 1))]


def test_every_byte_value_in_every_channel():
    p = np.arange(256, dtype=np.int64).reshape(16, 16)
    a = np.stack([np.stack([(p + 85 * c + 7 * i) % 256 for c in range(3)], axis=-1) for i in range(2)]).astype(np.uint8)
    assert all(len(np.unique(a[i, :, :, c])) == 256 for i in range(2) for c in range(3))
    for mean, std in ((0.5, 0.5), (0.25, 0.5)):
        _check([a], [1, 0], 0, 2, [(0, 0), (0, 1)], mean=mean, std=std)
        _check([a[:, :5, :7]], [1, 0], 0, 2, [(0, 0)], mean=mean, std=std)           # the scalar kernel's arithmetic


def test_partner_list_and_edit_render_groups():
    """The groups of the editing datasets: four edit renders per photo (index * 4 + t), and one drawn from the partner list."""
    photos, edits = _images('gpu/edit/p', 3, 8, 8), _images('gpu/edit/e', 12, 8, 8)
    order, partner = [2, 0, 1, 1], [9, 3, 6, 4]
    _check([photos, edits], order, 0, 4, [(0, 0)] + [(1, 0, 0, 4, t) for t in range(4)])
    _check([photos, photos, edits], order, 1, 3, [(0, 0), (1, 0), (2, 0, 1, 1, 0)], partner=partner, partner_limit=12)


def test_out_of_range_slots_are_skipped():
    """The raw entry does not check the index list; the kernel does: a slot whose image index, position or bank is out of
    range keeps what its output held (NaN here), and its neighbours are written."""
    from op import _native
    a = _images('gpu/skip/a', 4, 8, 8)
    bank = torch.from_numpy(a).to(gpumem.dev())
    index = torch.tensor([1, 4, -1, 3, 0], dtype=torch.int32, device=gpumem.dev())
    buf, view = gpumem.guarded((12, 3, 8, 8))
    groups = [(0, 0, 0, 1, 0), (2, 0, 0, 1, 0)]                # the second group names a bank that is not there
    _native.bank_gather([bank], index, None, 0, 6, 1, groups, out=view)      # member 5 is past the index list
    ref = torch.from_numpy(a).permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)
    got = view.cpu()
    for s, i in ((0, 1), (3, 3), (4, 0)):
        assert torch.equal(got[s], ref[i])
    for s in (1, 2, 5, 6, 7, 8, 9, 10, 11):
        assert bool(torch.isnan(got[s]).all()), s
    assert gpumem.guards_intact(buf)


def test_offsets_beyond_32_bits():
    """One bank of 21 846 images of 256 x 256 x 3 bytes, 4.29e9 bytes: image 10 923 is the first that starts past 2^31
    bytes, the last two lie past 2^32.  Only the four images gathered are written and read."""
    from op import image_bank
    from op.image_bank import ImageBank
    n = 21846
    assert n * 256 * 256 * 3 > 2 ** 32 and 10923 * 256 * 256 * 3 > 2 ** 31 > 10922 * 256 * 256 * 3
    which = [0, 10923, n - 2, n - 1]
    small = _images('gpu/large', 4, 256, 256)
    big = torch.empty((n, 256, 256, 3), dtype=torch.uint8, device=gpumem.dev())
    for k, i in enumerate(which):
        big[i].copy_(torch.from_numpy(small[k]))
    want = image_bank.bank_gather(_banks([small], 'cpu'), _index([3, 1, 0, 2], 4, 'cpu'), 0, 4, [(0, 0), (0, 1)])
    buf, view = gpumem.guarded(tuple(want.shape))
    index = _index([which[k] for k in (3, 1, 0, 2)], n, gpumem.dev())
    with launches.observed() as rec:
        got = image_bank.bank_gather([ImageBank(big)], index, 0, 4, [(0, 0), (0, 1)], out=view)
    assert torch.equal(got.cpu(), want) and gpumem.guards_intact(buf) and rec.names == ['bank_gather']
    del big, got
    torch.cuda.empty_cache()


def test_empty_batch_launches_nothing():
    from op import image_bank
    banks = _banks([_images('gpu/empty', 3, 8, 8)], gpumem.dev())
    with launches.observed() as rec:
        out = image_bank.bank_gather(banks, _index([0, 1], 3, gpumem.dev()), 2, 0, [(0, 0), (0, 0)])
    assert tuple(out.shape) == (0, 3, 8, 8) and out.dtype == torch.float32 and out.is_cuda and rec.seen == []


def test_launch_goes_on_the_current_stream():
    """Under torch.cuda.stream(side) the gather is ordered after the side stream's earlier work — the copy that fills the
    bank, behind a few hundred megabytes of fills — and only that stream is synchronised before comparing."""
    from op import image_bank
    from op.image_bank import ImageBank
    a = _images('gpu/stream', 8, 256, 256)
    src = torch.from_numpy(a).pin_memory()
    bank = torch.zeros(a.shape, dtype=torch.uint8, device=gpumem.dev())
    index = _index([7, 0, 3, 3, 5, 1, 6, 2], 8, gpumem.dev())
    want = image_bank.bank_gather(_banks([a], 'cpu'), _index([7, 0, 3, 3, 5, 1, 6, 2], 8, 'cpu'), 0, 8, [(0, 1)])
    ballast = torch.empty(64 << 20, dtype=torch.float32, device=gpumem.dev())
    buf, view = gpumem.guarded(tuple(want.shape))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for k in range(4):
            ballast.fill_(float(k))
        bank.copy_(src, non_blocking=True)
        got = image_bank.bank_gather([ImageBank(bank)], index, 0, 8, [(0, 1)], out=view)
    side.synchronize()
    assert torch.equal(got.cpu(), want) and gpumem.guards_intact(buf)
    torch.cuda.synchronize()


def test_switch_gives_the_same_bits_without_the_kernel(monkeypatch, real_arrays):
    from op import image_bank
    order = [20, 3, 3, 7, 0, 20, 11, 11]
    fused = _check(real_arrays, order, 0, 8, PAIR).clone()
    monkeypatch.setattr(image_bank, 'BANK_FUSE', False)
    plain = _check(real_arrays, order, 0, 8, PAIR, brackets=0)
    assert torch.equal(fused, plain)
    _check([_images('gpu/switch', 4, 5, 7)], [2, 3, 0, 1], 0, 4, [(0, 1)], mean=0.25, brackets=0)


def test_bank_loader_on_device_banks_equals_the_cpu_run():
    """BankLoader + Data_Loading over device banks against the same seeded run over CPU banks, across epoch boundaries:
    the epoch's list is uploaded once, then every batch is one launch and one allocation."""
    import dataset
    import train_3_encoder as T
    from torch.utils import data
    arrays = [_images('gpu/loader/g', 21, 8, 8), _images('gpu/loader/r', 21, 8, 8)]
    flags = [(False, False), (True, False), (True, True)] * 4

    def run(device):
        res = dataset.Resident.from_banks('pair', _banks(arrays, device))
        np.random.seed(5)

        def gen(seed):
            g = torch.Generator()
            g.manual_seed(seed)
            return g
        rec = T.sample_data(dataset.BankLoader(res, 6, data.RandomSampler(res, generator=gen(1))))
        ds_ = T.sample_data(dataset.BankLoader(res, 6, dataset.DualSupervisionSampler(res, 7, generator=gen(2))))
        ep = T.sample_data(dataset.BankLoader(res, 4, dataset.ExtremePoseDualSupervisionSampler(res, 7, generator=gen(3))))
        out = [dataset.Data_Loading(rec, ds_, f, device, extreme_loader=ep, extreme_ds_flag=e) for f, e in flags]
        plain = [next(rec) for _ in range(2)]
        return out, plain, res

    want, want_plain, _ = run(torch.device('cpu'))
    with launches.observed() as rec:
        got, got_plain, res = run(gpumem.dev())
    assert rec.names == ['bank_gather'] * (len(flags) + 2)
    for a, b in zip(got + got_plain, want + want_plain):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.is_cuda and x.is_contiguous() and torch.equal(x.cpu(), y)
    g_input, r_input, g_ref = got[0]
    assert g_ref.data_ptr() != g_input.data_ptr()
    assert g_input.untyped_storage().data_ptr() == r_input.untyped_storage().data_ptr() == g_ref.untyped_storage().data_ptr()
    g, r = res[20]
    assert torch.equal(g.cpu(), torch.from_numpy(arrays[0][20]).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5))
    assert torch.equal(r.cpu(), torch.from_numpy(arrays[1][20]).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5))


def test_bank_fill_on_the_device_equals_the_host_fill(tmp_path):
    """ImageBank.from_files onto the GPU — equally sized sources through the Pillow-exact resize kernel, unequal ones through
    Pillow on the host — holds the bytes of the fill on a CPU device, where Pillow resizes everything; a Resident over the
    files then yields the items of the dataset with Transform."""
    pytest.importorskip('PIL.Image')
    import dataset
    from op.image_bank import ImageBank
    dirs = C.write_tree(tmp_path)
    syn = dataset.Synthetic_Dataset(dirs['synface'], dataset.Transform(C.SIZE))
    mixed = dataset.FFHQ_Dataset(dirs['img']).images_list
    for paths in (syn.g_img_list, syn.r_img_list, mixed):
        host = ImageBank.from_files(paths, C.SIZE, 'cpu')
        for chunk in (256, 4):
            device = ImageBank.from_files(paths, C.SIZE, gpumem.dev(), chunk=chunk)
            assert device.data.is_cuda and torch.equal(device.data.cpu(), host.data)
    res = dataset.Resident(syn, C.SIZE, gpumem.dev())
    for i in (0, 10, 20):
        for a, b in zip(res[i], syn[i]):
            assert torch.equal(a.cpu(), b)
