"""Device-resident image banks and the batch gather over them.

A dataset at the model's size fits in HBM many times over (70 000 FFHQ photos at 256^2 are 13.8 GB of uint8), so the
images are decoded once into a bank, uint8 [N, H, W, 3] on the device, the epoch's index list is uploaded once, and every
batch — with the pair swap of the dual-supervision iterations folded into the indices — is one launch of
csrc/image_bank.hip that reads the bank and writes normalised float32 CHW.  No worker processes, no host-to-device copy
and no host synchronisation per iteration.

    ImageBank    the bytes: from_arrays / from_files (PIL decode + the reference's Resize, once) / save / load (.npy)
    EpochIndex   one epoch's index list (and, where an item needs one, its drawn partners) on the bank's device,
                 range-checked on the host when it is uploaded
    bank_gather  groups of images out of up to 4 banks in one launch; banks on a CPU device, or FMGAN_NO_BANK_FUSE=1,
                 take the composite: index_select plus the same arithmetic
"""
import os

import numpy as np
import torch

from op import _native

# FMGAN_NO_BANK_FUSE=1: bank_gather takes the composite form on the GPU too (index_select + images_to_tensor per group)
BANK_FUSE = os.environ.get('FMGAN_NO_BANK_FUSE', '0') != '1'
MAX_WORKERS = 16                      # decode threads of from_files: the CPU share of one rank, never os.cpu_count()
UPLOAD_BYTES = 256 << 20              # host -> device chunk of load()


def _as_u8_hwc(a):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f'ImageBank: expected uint8 [N, H, W, 3] images, got {a.dtype} {a.shape}')
    return a


class ImageBank:
    """uint8 [N, H, W, 3] images on one device."""

    def __init__(self, data):
        if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.ndim != 4 or data.shape[3] != 3 \
                or not data.is_contiguous():
            raise ValueError('ImageBank: data must be a contiguous uint8 [N, H, W, 3] tensor')
        self.data = data

    def __len__(self):
        return int(self.data.shape[0])

    @property
    def device(self):
        return self.data.device

    @property
    def size(self):
        return int(self.data.shape[1]), int(self.data.shape[2])

    @classmethod
    def from_arrays(cls, images, device='cpu'):
        """An array [N, H, W, 3], or a list of equally sized [H, W, 3] arrays (numpy or tensors), uint8."""
        if torch.is_tensor(images):
            data = images
        else:
            if isinstance(images, (list, tuple)):
                items = [t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in images]
                if len({i.shape for i in items}) > 1:
                    raise ValueError(f'ImageBank.from_arrays: images of unequal sizes {sorted({i.shape for i in items})}')
                images = np.stack(items) if items else np.zeros((0, 1, 1, 3), np.uint8)
            data = torch.from_numpy(np.ascontiguousarray(_as_u8_hwc(images)))
        return cls(data.to(device).contiguous())

    @classmethod
    def from_files(cls, paths, size, device='cpu', chunk=256, workers=8):
        """Decode `paths` once: PIL.Image.open(p).convert('RGB'), then the reference's Resize(size).  A chunk of equally
        sized sources is resized on a GPU `device` by Util.image_io.resize_images (Pillow's arithmetic, bit for bit);
        otherwise Pillow resizes on the host to Util.image_io.resize_output_size.  `workers` decode threads, at most
        MAX_WORKERS.  Unequal resulting sizes raise ValueError."""
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
        from Util import image_io
        device = torch.device(device)
        workers = max(1, min(int(workers), MAX_WORKERS))
        paths = list(paths)

        def decode(p):
            with Image.open(p) as im:
                return np.asarray(im.convert('RGB'))

        def host_resize(a):
            oh, ow = image_io.resize_output_size(a.shape[0], a.shape[1], size)
            if (oh, ow) == a.shape[:2]:
                return a
            return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))

        parts = []
        with ThreadPoolExecutor(workers) as pool:
            for c0 in range(0, len(paths), max(1, int(chunk))):
                items = list(pool.map(decode, paths[c0:c0 + chunk]))
                if device.type == 'cuda' and len({a.shape for a in items}) == 1:
                    part = image_io.resize_images(torch.from_numpy(np.stack(items)).to(device), size)
                else:
                    items = list(pool.map(host_resize, items))
                    if len({a.shape for a in items}) > 1:
                        raise ValueError(f'ImageBank.from_files: Resize({size}) leaves unequal sizes '
                                         f'{sorted({a.shape[:2] for a in items})}')
                    part = torch.from_numpy(np.stack(items)).to(device)
                if parts and part.shape[1:] != parts[0].shape[1:]:
                    raise ValueError(f'ImageBank.from_files: Resize({size}) leaves unequal sizes '
                                     f'{tuple(parts[0].shape[1:3])} and {tuple(part.shape[1:3])}')
                parts.append(part)
        if not parts:
            return cls(torch.zeros((0, size, size, 3), dtype=torch.uint8, device=device))
        return cls(torch.cat(parts).contiguous() if len(parts) > 1 else parts[0].contiguous())

    def save(self, path):
        """A plain .npy of the bytes: a folder is then decoded once, not once per run."""
        with open(path, 'wb') as f:
            np.save(f, self.data.cpu().numpy())

    @classmethod
    def load(cls, path, device='cpu'):
        """Read what save() wrote, through a memory map, uploading UPLOAD_BYTES at a time."""
        a = _as_u8_hwc(np.load(path, mmap_mode='r'))
        data = torch.empty(a.shape, dtype=torch.uint8, device=device)
        per = max(1, UPLOAD_BYTES // max(1, int(np.prod(a.shape[1:]))))
        for i0 in range(0, a.shape[0], per):
            data[i0:i0 + per].copy_(torch.from_numpy(np.array(a[i0:i0 + per])))      # a writable copy of the mapped pages
        return cls(data)


class EpochIndex:
    """One epoch's index list on the device: `indices` (ints in [0, limit)) and, where an item needs a drawn partner,
    `partner` (ints in [0, partner_limit), one per entry).  Checked here, on the host, once: IndexError."""

    def __init__(self, indices, limit, device, partner=None, partner_limit=None):
        self.limit = int(limit)
        self.data = self._upload(indices, self.limit, device, 'index')
        self.partner, self.partner_limit = None, None
        if partner is not None:
            self.partner_limit = int(partner_limit)
            self.partner = self._upload(partner, self.partner_limit, device, 'partner index')
            if self.partner.numel() != self.data.numel():
                raise IndexError(f'EpochIndex: {self.partner.numel()} partners for {self.data.numel()} indices')

    @staticmethod
    def _upload(values, limit, device, what):
        a = np.asarray(values, dtype=np.int64).reshape(-1)
        if a.size and (int(a.min()) < 0 or int(a.max()) >= limit):
            bad = a[(a < 0) | (a >= limit)][0]
            raise IndexError(f'EpochIndex: {what} {int(bad)} is out of range for {limit} items')
        return torch.from_numpy(a.astype(np.int32)).to(device)

    def __len__(self):
        return int(self.data.numel())


def _tensor_of(bank):
    return bank.data if isinstance(bank, ImageBank) else bank


def check_banks(banks):
    """dtype, layout, device and equal H x W of `banks` (ImageBanks or tensors), on the host: the tensors."""
    tensors = [_tensor_of(b) for b in banks]
    if not 1 <= len(tensors) <= _native.BANK_GATHER_BANKS:
        raise ValueError(f'bank_gather: {len(tensors)} banks, 1..{_native.BANK_GATHER_BANKS} are served')
    first = tensors[0]
    for k, t in enumerate(tensors):
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.ndim != 4 or t.shape[3] != 3:
            raise ValueError(f'bank_gather: banks[{k}] must be a uint8 [N, H, W, 3] tensor, got '
                             f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
        if not t.is_contiguous():
            raise ValueError(f'bank_gather: banks[{k}] must be contiguous, got strides {t.stride()}')
        if t.device != first.device:
            raise RuntimeError(f'bank_gather: banks[{k}] is on {t.device}, banks[0] on {first.device}')
        if tuple(t.shape[1:3]) != tuple(first.shape[1:3]):
            raise ValueError(f'bank_gather: banks[{k}] holds {tuple(t.shape[1:3])} images, banks[0] '
                             f'{tuple(first.shape[1:3])}')
    return tensors


def bank_gather(banks, index, offset, batch, groups, even_only=False, mean=0.5, std=0.5, out=None):
    """Groups of normalised images out of `banks` for the `batch` positions offset .. offset + batch of `index`.

    groups: one (bank, swap) or (bank, swap, source, mul, add) per output group.  Member b of a group is image
    index[b ^ swap] * mul + add of banks[bank] (source 1: index.partner instead of the index list; mul, add default to
    1, 0); swap 1 is the reference's Swap_List_Pair.  even_only keeps the even members b = 0, 2, ...
    Returns float32 [len(groups) * members, 3, H, W] = ((image / 255) - mean) / std, group after group, members = batch
    or batch // 2: one allocation, so each group is a contiguous view of it.  On GPU banks one launch on the current
    stream (one `bank_gather` bracket); CPU banks and FMGAN_NO_BANK_FUSE=1 take the composite.
    Everything is checked on the host before any launch: ValueError / RuntimeError for banks, groups and `out`,
    IndexError for positions beyond the index list, an odd batch with a swap or even_only, and a group whose images
    index * mul + add can leave its bank."""
    tensors = check_banks(banks)
    device = tensors[0].device
    if not isinstance(index, EpochIndex):
        raise ValueError('bank_gather: index must be an EpochIndex (the epoch\'s list, uploaded once)')
    if index.data.device != device:
        raise RuntimeError(f'bank_gather: the index is on {index.data.device}, the banks on {device}')
    offset, batch = int(offset), int(batch)
    full = []
    for g in groups:
        g = tuple(int(v) for v in g)
        if len(g) == 2:
            g = g + (0, 1, 0)
        if len(g) != 5 or g[1] not in (0, 1) or g[2] not in (0, 1) or not 0 <= g[0] < len(tensors):
            raise ValueError(f'bank_gather: group {g}: (bank, swap) or (bank, swap, source, mul, add) with bank below '
                             f'{len(tensors)} and swap, source in (0, 1)')
        bank, swap, source, mul, add = g
        if source == 1 and index.partner is None:
            raise ValueError('bank_gather: a group reads the partner list and the index has none')
        limit = index.partner_limit if source == 1 else index.limit
        lo, hi = sorted((add, (limit - 1) * mul + add)) if limit > 0 else (0, 0)
        if lo < 0 or hi >= tensors[bank].shape[0]:
            raise IndexError(f'bank_gather: group {g} reaches images {lo} .. {hi} of a bank of {tensors[bank].shape[0]}')
        full.append((bank, source, swap, mul, add))
    if not 1 <= len(full) <= _native.BANK_GATHER_GROUPS:
        raise ValueError(f'bank_gather: {len(full)} groups, 1..{_native.BANK_GATHER_GROUPS} are served')
    if offset < 0 or batch < 0 or offset + batch > len(index):
        raise IndexError(f'bank_gather: positions {offset} .. {offset + batch} of an index list of {len(index)}')
    if batch % 2 and (even_only or any(g[2] for g in full)):
        raise IndexError('bank_gather: odd batch with a pair swap')
    if float(std) == 0.0:
        raise ValueError('bank_gather: std must not be 0')
    stride = 2 if even_only else 1
    members = batch // stride
    h, w = int(tensors[0].shape[1]), int(tensors[0].shape[2])
    shape = (len(full) * members, 3, h, w)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != device \
                or not out.is_contiguous():
            raise ValueError(f'bank_gather: out must be a contiguous float32 {shape} tensor on {device}')
    if device.type == 'cuda' and BANK_FUSE:
        return _native.bank_gather(tensors, index.data, index.partner, offset, members, stride, full, mean, std, out)
    return _composite(tensors, index, offset, batch, stride, full, mean, std, out, shape)


def _composite(tensors, index, offset, batch, stride, groups, mean, std, out, shape):
    """index_select plus the same arithmetic, group by group: torch's on a CPU device (IEEE division and subtraction in
    float32, the order of ToTensor + Normalize), Util.image_io.images_to_tensor on a GPU."""
    device = tensors[0].device
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    members = batch // stride
    if members == 0:
        return out
    b = torch.arange(0, batch, stride, device=device)
    for k, (bank, source, swap, mul, add) in enumerate(groups):
        src = index.partner if source == 1 else index.data
        i = src[offset + (b ^ swap)].long() * mul + add
        images = tensors[bank].index_select(0, i)
        if device.type == 'cuda':
            t = _native.images_to_tensor(images, mean, std)
        else:
            t = images.permute(0, 3, 1, 2).to(torch.float32).div(255).sub(float(mean)).div(float(std))
        out[k * members:(k + 1) * members].copy_(t)
    return out
