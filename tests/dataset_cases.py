"""Cases shared by tests/test_dataset.py, tests/test_dataset_gpu.py and tools/make_golden_dataset.py (which records
tests/golden/dataset.npz from the reference's dataset.py over the same tree and the same seeds)."""
import os

import numpy as np

N_IMG_PER_ID = 7
SAMPLER_LENS = (21, 70)                     # len(data_source): 3 and 10 identities of 7 images
SAMPLER_SEED = {21: (11, 5), 70: (12, 6)}   # len -> (np.random.seed, torch.Generator seed)
SIZE = 8                                    # Resize(SIZE) of the tree below
IDS = ('id_1', 'id_10', 'id_2')             # plain string order puts id_10 before id_2
N_PHOTOS = 6


class Sized:
    """A data source of which the samplers only ask the length."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def image(tag, h, w, channels=3):
    """Deterministic uint8 image [h, w, channels] ([h, w] for channels = 1); every byte value occurs over the tree."""
    import zlib
    rng = np.random.RandomState(zlib.crc32(tag.encode()) & 0x7fffffff)
    a = rng.randint(0, 256, size=(h, w, channels)).astype(np.uint8)
    return a[:, :, 0] if channels == 1 else a


def write_tree(root):
    """The folder tree of the file-list and loader tests, as PNG files under `root`:
      synface/<id>/{g,r}_<v>.png   3 identities x 7 variations, 12 x 12 (-> 8 x 8); one RGBA and one greyscale file, and in
                                   id_2 a file whose name matches neither 'g_' nor 'r_'
      ffhq/{img,render_img}/       6 files each, 12 x 12 and 24 x 24 mixed (both -> 8 x 8: the host resize of unequal sources)
      ffhq/edit_render_img/        24 files, four per photo
    Returns the dict of the sub-folders."""
    from PIL import Image
    root = str(root)
    syn = os.path.join(root, 'synface')
    for pid in IDS:
        os.makedirs(os.path.join(syn, pid))
        for v in range(N_IMG_PER_ID):
            for kind in 'gr':
                name = f'{kind}_{v}.png'
                if (pid, kind, v) == ('id_10', 'g', 3):
                    im = Image.fromarray(image(f'{pid}/{name}', 12, 12, 4), 'RGBA')
                elif (pid, kind, v) == ('id_2', 'r', 5):
                    im = Image.fromarray(image(f'{pid}/{name}', 12, 12, 1), 'L')
                else:
                    im = Image.fromarray(image(f'{pid}/{name}', 12, 12))
                im.save(os.path.join(syn, pid, name))
    Image.fromarray(image('id_2/contact_sheet', 5, 5)).save(os.path.join(syn, 'id_2', 'contact_sheet.png'))
    ffhq = os.path.join(root, 'ffhq')
    for sub, n in (('img', N_PHOTOS), ('render_img', N_PHOTOS), ('edit_render_img', 4 * N_PHOTOS)):
        os.makedirs(os.path.join(ffhq, sub))
        for i in range(n):
            side = 24 if i % 3 == 1 else 12
            # unpadded numbers: 11.png sorts before 4.png as a string, and the order of writing is neither
            Image.fromarray(image(f'{sub}/{i}', side, side)).save(os.path.join(ffhq, sub, f'{(i * 7) % 31}.png'))
    return {'synface': syn, 'img': os.path.join(ffhq, 'img'), 'render_img': os.path.join(ffhq, 'render_img'),
            'edit_render_img': os.path.join(ffhq, 'edit_render_img')}


def build_datasets(mod, dirs, transform=None):
    """The four dataset classes of module `mod` (this package's dataset.py or the reference's) over write_tree's dirs."""
    return {
        'ffhq': mod.FFHQ_Dataset(dirs['img'], transform),
        'synthetic': mod.Synthetic_Dataset(dirs['synface'], transform),
        'reconstruction': mod.FFHQ_Dataset_Reconstruction(dirs['img'], dirs['render_img'], transform),
        'editing': mod.FFHQ_Dataset_Editing(dirs['img'], dirs['edit_render_img'], transform, train=False),
        'editing_train': mod.FFHQ_Dataset_Editing(dirs['img'], dirs['edit_render_img'], transform, train=True,
                                                  render_image_folder=dirs['render_img']),
    }


def file_lists(ds):
    """name -> the flat file list(s) of a dataset, in the order its class keeps them."""
    kind = type(ds).__name__
    if kind == 'FFHQ_Dataset':
        return {'images': ds.images_list}
    if kind == 'Synthetic_Dataset':
        return {'ids': ds.id_list, 'g': ds.g_img_list, 'r': ds.r_img_list}
    if kind == 'FFHQ_Dataset_Reconstruction':
        return {'photo': ds.photo_image_list, 'render': ds.render_image_list}
    out = {'photo': ds.photo_image_list, 'edit': [f for group in ds.edit_render_image_list for f in group]}
    if ds.train:
        out['render'] = ds.render_image_list
    return out


def relative(paths, root):
    return [os.path.relpath(p, str(root)).replace(os.sep, '/') for p in paths]


EDIT_TRAIN_SEED = 21        # np.random.seed before the items of 'editing_train' are read, item 0 upwards


def item_arrays(item):
    """The PIL images of one transform=None item as a list of uint8 arrays."""
    items = item if isinstance(item, (list, tuple)) else [item]
    return [np.array(im) for im in items]
