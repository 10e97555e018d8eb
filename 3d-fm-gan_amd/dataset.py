"""The data side of train() (reference: dataset.py): dataset classes, the two dual-supervision samplers, and batch
assembly either side of the path.

The reference reads its folders through four DataLoaders with 8 worker processes each: PIL decode plus Resize / ToTensor
/ Normalize per item per iteration, float32 batches over PCIe, and the pair swap as a Python list + a numpy round trip
through host memory (`g_input.detach().cpu().numpy()[swap_list]`).  The datasets at the model's size fit in HBM many
times over, so here:

    FFHQ_Dataset, Synthetic_Dataset, FFHQ_Dataset_Reconstruction, FFHQ_Dataset_Editing
                   the reference's classes: same constructor arguments, same file lists in the same order, same items
    DualSupervisionSampler, ExtremePoseDualSupervisionSampler (+ the two list augmentations)
                   the same draws from torch.randperm and np.random.choice in the same order
    Transform      Resize + ToTensor + Normalize on a PIL image (the non-resident path and the sample pickers)
    Resident       the images of one dataset decoded once into uint8 banks on the device (op/image_bank.py)
    BankLoader     batches of a Resident for any sampler: the batches of BatchSampler(sampler, batch_size, drop_last), the
                   tensors a DataLoader would yield, each batch one HIP launch reading the bank; training_batch() is the
                   (g_input, r_input, g_ref) triple of Data_Loading with the pair swap folded into the indices
    Data_Loading   one training batch from whichever loaders it is given

A loader that yields plain (photo, render) batches takes the swap as one index_select on whatever device the batch lives.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset, Sampler

from op import image_bank
from op.image_bank import EpochIndex, ImageBank

N_EDIT_IMG_PER_ID = 4          # edit renders per photo of FFHQ_Dataset_Editing (dataset.py:117)


# ----------------------------------------------------------------------------------------------- transform
class Transform:
    """transforms.Compose([Resize(size), ToTensor(), Normalize((mean,)*3, (std,)*3)]) (train_3_encoder.py:233-239) on a PIL
    image, without torchvision: PIL's bilinear resize to Util.image_io.resize_output_size, then ((x / 255) - mean) / std
    as float32 CHW — the arithmetic of the device path, bit for bit."""

    def __init__(self, size, mean=0.5, std=0.5):
        self.size, self.mean, self.std = int(size), float(mean), float(std)

    def __call__(self, img):
        from PIL import Image
        from Util import image_io
        w, h = img.size
        oh, ow = image_io.resize_output_size(h, w, self.size)
        if (oh, ow) != (h, w):
            img = img.resize((ow, oh), Image.BILINEAR)
        a = np.array(img)
        if a.ndim == 2:
            a = a[:, :, None]
        t = torch.from_numpy(a).permute(2, 0, 1).contiguous()
        return t.to(torch.float32).div(255).sub_(self.mean).div_(self.std)


def _open_rgb(path):
    from PIL import Image
    return Image.open(path).convert('RGB')


def _listed(folder):
    return [os.path.join(folder, name) for name in sorted(os.listdir(folder))]


# ----------------------------------------------------------------------------------------------- dataset classes
class FFHQ_Dataset(Dataset):
    """The photos of one folder, in sorted order (dataset.py:19-39)."""

    def __init__(self, image_folder, transform=None):
        self.images_list = _listed(image_folder)
        self.transform = transform

    def __getitem__(self, index):
        img = _open_rgb(self.images_list[index])
        return img if self.transform is None else self.transform(img)

    def __len__(self):
        return len(self.images_list)


class Synthetic_Dataset(Dataset):
    """(generated image, render) pairs of a DiscoFaceGAN tree, one folder per identity (dataset.py:42-74): identities and
    the files of each in sorted order (plain string order: id_10 before id_2), files selected by the substrings 'g_' /
    'r_' of their names."""

    def __init__(self, image_folder, transform=None):
        self.id_list = sorted(os.listdir(image_folder))
        self.g_img_list, self.r_img_list = [], []
        for pid in self.id_list:
            id_dir = os.path.join(image_folder, pid)
            names = sorted(os.listdir(id_dir))
            self.g_img_list += [os.path.join(id_dir, n) for n in names if 'g_' in n]
            self.r_img_list += [os.path.join(id_dir, n) for n in names if 'r_' in n]
        self.transform = transform

    def __getitem__(self, index):
        g_img, r_img = _open_rgb(self.g_img_list[index]), _open_rgb(self.r_img_list[index])
        if self.transform is not None:
            g_img, r_img = self.transform(g_img), self.transform(r_img)
        return g_img, r_img

    def __len__(self):
        return len(self.g_img_list)


class FFHQ_Dataset_Reconstruction(Dataset):
    """(photo, render) pairs from two folders of equally many files, each in sorted order (dataset.py:76-106)."""

    def __init__(self, photo_image_folder, render_image_folder, transform=None):
        self.photo_image_list = _listed(photo_image_folder)
        self.render_image_list = _listed(render_image_folder)
        assert len(self.photo_image_list) == len(self.render_image_list)
        self.transform = transform

    def __getitem__(self, index):
        photo_img, render_img = _open_rgb(self.photo_image_list[index]), _open_rgb(self.render_image_list[index])
        if self.transform is not None:
            photo_img, render_img = self.transform(photo_img), self.transform(render_img)
        return photo_img, render_img

    def __len__(self):
        return len(self.photo_image_list)


class FFHQ_Dataset_Editing(Dataset):
    """A photo with its N_EDIT_IMG_PER_ID edit renders (dataset.py:109-160): item i is [photo, the four edit renders]
    for the quantitative editing evaluation, or with train=True [photo, its own render, ONE edit render drawn with
    np.random.choice] for self-supervised contrastive training.  edit_render_image_list[i] are the four files of photo i
    (files 4i .. 4i + 3 of the sorted folder)."""

    def __init__(self, photo_image_folder, edit_render_image_folder, transform=None, train=False, render_image_folder=None):
        self.photo_image_list = _listed(photo_image_folder)
        flat = _listed(edit_render_image_folder)
        assert len(self.photo_image_list) * N_EDIT_IMG_PER_ID == len(flat)
        self.edit_render_image_list = [flat[N_EDIT_IMG_PER_ID * i:N_EDIT_IMG_PER_ID * (i + 1)]
                                       for i in range(len(self.photo_image_list))]
        if train:
            self.render_image_list = _listed(render_image_folder)
            assert len(self.render_image_list) == len(self.photo_image_list)
        self.transform = transform
        self.train = train

    def __getitem__(self, index):
        edit_files = self.edit_render_image_list[index]
        photo_img = _open_rgb(self.photo_image_list[index])
        if self.train:
            edit_file = np.random.choice(edit_files)
            render_img_list = [_open_rgb(f) for f in (self.render_image_list[index], edit_file)]
        else:
            render_img_list = [_open_rgb(f) for f in edit_files]
        if self.transform is not None:
            photo_img = self.transform(photo_img)
            render_img_list = [self.transform(r) for r in render_img_list]
        return [photo_img] + render_img_list

    def __len__(self):
        return len(self.photo_image_list)


# ----------------------------------------------------------------------------------------------- samplers
def dual_supervision_list_augmentation(index_list, n_img_per_id):
    """[i, ...] -> [i, partner(i), ...] (dataset.py:166-191): the partner is another image of i's identity (images
    n_img_per_id * p .. n_img_per_id * p + n_img_per_id - 1 belong to identity p), drawn with np.random.choice from the
    other n_img_per_id - 1 variations.  Entries 2j and 2j + 1 are a dual-supervision pair."""
    dual_index_list = []
    for idx in index_list:
        person_id, var_id = idx // n_img_per_id, idx % n_img_per_id
        dual_var_id = np.random.choice([i for i in range(n_img_per_id) if i != var_id])
        dual_index_list += [idx, person_id * n_img_per_id + dual_var_id]
    return dual_index_list


def extreme_pose_list_augmentation(index_list, n_img_per_id):
    """Identity indices [p, ...] -> image indices [normal pose of p, an extreme pose of p, ...] (dataset.py:310-337):
    image n_img_per_id * p is the normal pose, the extreme one is drawn with np.random.choice from the offsets
    1 .. n_img_per_id - 1."""
    extreme_idx_list = []
    for index in index_list:
        normal_pose_index = index * n_img_per_id
        extreme_idx_list.append(normal_pose_index)
        extreme_idx_list.append(normal_pose_index + np.random.choice(np.arange(1, n_img_per_id)))
    return extreme_idx_list


class _PairSampler(Sampler):
    """What the reference's two samplers share (dataset.py:194-307): the constructor checks of torch's RandomSampler, a
    torch.randperm(generator=...) of `_population()` entries, and its augmentation to twice as many image indices."""

    def __init__(self, data_source, n_img_per_id, replacement=False, num_samples=None, generator=None):
        self.data_source = data_source
        self.n_img_per_id = n_img_per_id
        self.replacement = replacement
        self._num_samples = num_samples
        self.generator = generator
        if not isinstance(self.replacement, bool):
            raise TypeError('replacement should be a boolean value, but got replacement={}'.format(self.replacement))
        if self._num_samples is not None and not replacement:
            raise ValueError('With replacement=False, num_samples should not be specified, since a random permute will '
                             'be performed.')
        if not isinstance(self.num_samples, int) or self.num_samples <= 0:
            raise ValueError('num_samples should be a positive integer value, but got num_samples={}'.format(
                self.num_samples))

    @property
    def num_samples(self):
        if self._num_samples is None:
            return self._default_num_samples()       # the dataset's size might change at run time
        return self._num_samples

    def __iter__(self):
        if self.generator is None:
            generator = torch.Generator()
            generator.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        else:
            generator = self.generator
        index_list = torch.randperm(self._population(), generator=generator).tolist()
        yield from self._augment(index_list)

    def __len__(self):
        return self.num_samples


class DualSupervisionSampler(_PairSampler):
    """A random permutation of the images, each followed by a partner of its identity (dataset.py:194-248)."""

    def _population(self):
        return len(self.data_source)

    def _default_num_samples(self):
        return 2 * len(self.data_source)

    def _augment(self, index_list):
        return dual_supervision_list_augmentation(index_list, self.n_img_per_id)


class ExtremePoseDualSupervisionSampler(_PairSampler):
    """A random permutation of the identities, each as (normal pose, an extreme pose) (dataset.py:254-307)."""

    def _population(self):
        return len(self.data_source) // self.n_img_per_id

    def _default_num_samples(self):
        return 2 * len(self.data_source) // self.n_img_per_id

    def _augment(self, index_list):
        return extreme_pose_list_augmentation(index_list, self.n_img_per_id)


# ----------------------------------------------------------------------------------------------- resident datasets
def _file_lists(dataset):
    """(kind, the file list of each bank) of one of the four dataset classes."""
    if isinstance(dataset, FFHQ_Dataset_Editing):
        flat = [f for files in dataset.edit_render_image_list for f in files]
        if dataset.train:
            return 'edit_train', [dataset.photo_image_list, dataset.render_image_list, flat]
        return 'edit_eval', [dataset.photo_image_list, flat]
    if isinstance(dataset, FFHQ_Dataset_Reconstruction):
        return 'pair', [dataset.photo_image_list, dataset.render_image_list]
    if isinstance(dataset, Synthetic_Dataset):
        return 'pair', [dataset.g_img_list, dataset.r_img_list]
    if isinstance(dataset, FFHQ_Dataset):
        return 'single', [dataset.images_list]
    raise TypeError(f'Resident: no bank layout for {type(dataset).__name__}')


# gather groups (bank, swap, source, mul, add) of a plain batch, per kind
_PLAIN_GROUPS = {
    'single': [(0, 0)],
    'pair': [(0, 0), (1, 0)],
    'edit_eval': [(0, 0)] + [(1, 0, 0, N_EDIT_IMG_PER_ID, t) for t in range(N_EDIT_IMG_PER_ID)],
    'edit_train': [(0, 0), (1, 0), (2, 0, 1, 1, 0)],        # the edit render comes from the drawn partner list
}


class Resident:
    """The images of one dataset in uint8 banks on `device`, decoded and resized once (ImageBank.from_files): 1 bank for
    FFHQ_Dataset, 2 for Synthetic_Dataset and FFHQ_Dataset_Reconstruction, 2 for FFHQ_Dataset_Editing (photos; edit
    renders, four per photo) or 3 with train=True (photos, renders, edit renders).  resident[i] is what dataset[i] with
    Transform(size) returns, on the device, so the sample pickers of Evaluation/visual_eval.py work on it unchanged.

    cache: a path prefix; bank k is kept as `{cache}.{k}.npy` and read from there when the file exists.
    share: a dict; banks of the same file list and size are built once for all Residents that are given it."""

    def __init__(self, dataset, size, device, cache=None, share=None, chunk=256, workers=8, mean=0.5, std=0.5):
        self.kind, lists = _file_lists(dataset)
        self.size, self.device, self.mean, self.std = int(size), torch.device(device), float(mean), float(std)
        self.banks = []
        for k, paths in enumerate(lists):
            key = (tuple(paths), self.size, str(self.device))
            bank = share.get(key) if share is not None else None
            if bank is None:
                file = None if cache is None else f'{cache}.{k}.npy'
                if file is not None and os.path.exists(file):
                    bank = ImageBank.load(file, self.device)
                    if len(bank) != len(paths):
                        raise ValueError(f'Resident: {file} holds {len(bank)} images, the dataset lists {len(paths)}')
                else:
                    bank = ImageBank.from_files(paths, self.size, self.device, chunk=chunk, workers=workers)
                    if file is not None:
                        bank.save(file)
                if share is not None:
                    share[key] = bank
            self.banks.append(bank)
        self._check()

    @classmethod
    def from_banks(cls, kind, banks, mean=0.5, std=0.5):
        """A Resident over banks that exist already (ImageBanks or uint8 [N, H, W, 3] tensors), `kind` one of 'single',
        'pair', 'edit_eval', 'edit_train'."""
        self = cls.__new__(cls)
        self.kind = kind
        self.banks = [b if isinstance(b, ImageBank) else ImageBank(b) for b in banks]
        self.size, self.device, self.mean, self.std = self.banks[0].size[0], self.banks[0].device, float(mean), float(std)
        self._check()
        return self

    def _check(self):
        want = {'single': 1, 'pair': 2, 'edit_eval': 2, 'edit_train': 3}
        if self.kind not in want or len(self.banks) != want[self.kind]:
            raise ValueError(f'Resident: kind {self.kind!r} with {len(self.banks)} banks')
        image_bank.check_banks(self.banks)
        n = len(self.banks[0])
        counts = [n] * len(self.banks)
        counts[-1] = n * N_EDIT_IMG_PER_ID if self.kind.startswith('edit') else n
        if [len(b) for b in self.banks] != counts:
            raise ValueError(f'Resident: banks of {[len(b) for b in self.banks]} images, expected {counts}')

    def __len__(self):
        return len(self.banks[0])

    def _image(self, bank, i):
        u8 = self.banks[bank].data[i:i + 1]
        if u8.is_cuda:
            from op import _native
            return _native.images_to_tensor(u8, self.mean, self.std)[0]
        return u8[0].permute(2, 0, 1).to(torch.float32).div(255).sub_(self.mean).div_(self.std)

    def __getitem__(self, index):
        i = int(index)
        if not -len(self) <= i < len(self):
            raise IndexError(f'Resident: index {i} of {len(self)} items')
        i %= len(self)
        if self.kind == 'single':
            return self._image(0, i)
        if self.kind == 'pair':
            return self._image(0, i), self._image(1, i)
        if self.kind == 'edit_train':
            edit = N_EDIT_IMG_PER_ID * i + int(np.random.choice(N_EDIT_IMG_PER_ID))
            return [self._image(0, i), self._image(1, i), self._image(2, edit)]
        return [self._image(0, i)] + [self._image(1, N_EDIT_IMG_PER_ID * i + t) for t in range(N_EDIT_IMG_PER_ID)]


class BankLoader:
    """Iterates a Resident as DataLoader(dataset, batch_size, sampler=sampler, drop_last=drop_last) would: the batches
    are those of BatchSampler(sampler, batch_size, drop_last), and a batch is `photo` for FFHQ_Dataset, `(photo,
    render)` for the paired datasets and `[photo, r_1, ...]` for FFHQ_Dataset_Editing, float32 on the bank's device.
    iter(loader) starts an epoch: list(sampler) is materialised, range-checked and uploaded once (with train=True
    editing data, also the epoch's np.random.choice draws of one edit render per item, in item order); after that a
    batch is one launch.  `indices` holds the dataset indices of the batch handed out last."""

    def __init__(self, resident, batch_size, sampler, drop_last=False):
        if not isinstance(batch_size, int) or isinstance(batch_size, bool) or batch_size <= 0:
            raise ValueError(f'batch_size should be a positive integer value, but got batch_size={batch_size}')
        self.resident, self.batch_size, self.sampler, self.drop_last = resident, batch_size, sampler, bool(drop_last)
        self.indices = None
        self._index = None

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = [int(i) for i in self.sampler]
        used = len(order) // self.batch_size * self.batch_size if self.drop_last else len(order)
        order = order[:used]
        r = self.resident
        partner = limit = None
        if r.kind == 'edit_train':
            limit = len(r.banks[2])
            # IndexError for an index outside the dataset before it reaches the partner arithmetic
            EpochIndex._upload(order, len(r), 'cpu', 'index')
            partner = [N_EDIT_IMG_PER_ID * i + int(np.random.choice(N_EDIT_IMG_PER_ID)) for i in order]
        self._index = EpochIndex(order, len(r), r.device, partner=partner, partner_limit=limit)
        self._order, self._cursor = order, 0
        return self

    def _take(self):
        if self._index is None:
            iter(self)
        if self._cursor >= len(self._order):
            self._index = None
            raise StopIteration
        offset = self._cursor
        n = min(self.batch_size, len(self._order) - offset)
        self._cursor += n
        self.indices = self._order[offset:offset + n]
        return offset, n

    def _gather(self, offset, n, groups, even_only=False):
        r = self.resident
        out = image_bank.bank_gather(r.banks, self._index, offset, n, groups, even_only=even_only, mean=r.mean,
                                     std=r.std)
        m = out.shape[0] // len(groups)
        return [out[k * m:(k + 1) * m] for k in range(len(groups))]

    def __next__(self):
        offset, n = self._take()
        parts = self._gather(offset, n, _PLAIN_GROUPS[self.resident.kind])
        if self.resident.kind == 'single':
            return parts[0]
        return tuple(parts) if self.resident.kind == 'pair' else parts

    def training_batch(self, pair=False, even_only=False):
        """(g_input, r_input, g_ref) of the next batch, from one launch (paired datasets only).  pair=False, a
        reconstruction batch: (photo, render, a second copy of the photo).  pair=True, dual supervision: (photo, the
        PARTNER's render, the partner's photo), the partner of member b being member b ^ 1; with even_only the even
        members alone, half the batch.  An odd batch with pair or even_only raises IndexError."""
        if self.resident.kind != 'pair':
            raise TypeError(f'training_batch: a (photo, render) dataset is needed, this one is {self.resident.kind!r}')
        if even_only and not pair:
            raise ValueError('training_batch: even_only goes with pair=True')
        offset, n = self._take()
        swap = 1 if pair else 0
        return tuple(self._gather(offset, n, [(0, 0), (1, swap), (0, swap)], even_only=even_only))


# ----------------------------------------------------------------------------------------------- batch assembly
def Swap_List_Pair(idx_list):
    """[0, 1, 2, 3, ...] -> [1, 0, 3, 2, ...] (dataset.py:343-358); the length must be even."""
    idx_list = list(idx_list)
    if len(idx_list) % 2:
        raise IndexError('Swap_List_Pair: odd number of items')
    return [idx_list[i ^ 1] for i in range(len(idx_list))]


def _swap_pairs(t):
    n = t.shape[0]
    if n % 2:
        raise IndexError('pair swap: odd batch')
    idx = torch.arange(n, device=t.device) ^ 1
    return t.index_select(0, idx)


def Data_Loading(rec_loader, ds_loader, ds_flag, device, extreme_loader=None, extreme_ds_flag=False,
                 pure_ffhq_loader=None, ds_dataset_type=None):
    """One training batch (dataset.py:361-413).  ds_dataset_type None:
    reconstruction   -> (photo, render, target = photo)
    dual supervision -> (photo, render of the PARTNER image, target = partner photo)
    extreme pose     -> the same, keeping only the even members of each pair.
    A loader with training_batch (BankLoader, bare or behind train_3_encoder.sample_data) assembles the triple itself, in
    one launch; any other loader yields (photo, render) batches, which are moved to `device` first, then permuted there.
    ds_dataset_type 'FFHQ': (photo, render, edit render, target = photo, a pure FFHQ batch), whatever the flags."""
    if ds_dataset_type == 'FFHQ':
        ffhq_ref = next(pure_ffhq_loader)
        g_input, r_input, r_edit_input = next(ds_loader)
        g_input = g_input.to(device)
        return g_input, r_input.to(device), r_edit_input.to(device), g_input.clone(), ffhq_ref.to(device)
    if ds_dataset_type is not None:
        raise ValueError(f'Data_Loading: ds_dataset_type {ds_dataset_type!r}: None or \'FFHQ\'')
    loader = rec_loader if not ds_flag else (extreme_loader if extreme_ds_flag else ds_loader)
    if hasattr(loader, 'training_batch'):
        g_input, r_input, g_ref = loader.training_batch(pair=bool(ds_flag), even_only=bool(ds_flag and extreme_ds_flag))
        return g_input.to(device), r_input.to(device), g_ref.to(device)
    if not ds_flag:
        g_input, r_input = next(rec_loader)
        g_input, r_input = g_input.to(device), r_input.to(device)
        return g_input, r_input, g_input.clone()
    g_input, r_input = next(loader)
    g_input, r_input = g_input.to(device), r_input.to(device)
    r_input = _swap_pairs(r_input)
    g_ref = _swap_pairs(g_input)
    if extreme_ds_flag:
        g_input, r_input, g_ref = g_input[0::2], r_input[0::2], g_ref[0::2]
    return g_input, r_input, g_ref
