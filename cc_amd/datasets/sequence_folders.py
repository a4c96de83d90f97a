"""The reference's training set on the host (datasets/sequence_folders.py): a root directory with `train.txt` / `val.txt` naming one
scene directory per line, each scene holding `cam.txt` (the 3x3 intrinsics, nine comma-separated values) and its frames as `*.jpg`.
A sample is a centre frame with its (sequence_length - 1) / 2 neighbours on either side; `SequenceFolder` keeps the reference's
constructor, its seeding (`random` and `np.random`), its `random.shuffle` of the samples -- the same seed gives the same sample
order -- and its return tuple.  `scipy.misc.imread` (gone from SciPy) is Pillow's decoder, which is what it called."""
import fnmatch
import os
import random

import numpy as np
import torch.utils.data as data


def crawl(root, train=True, sequence_length=3):
    """-> (scenes, intrinsics, samples): the scene names of train.txt / val.txt in file order, float32 [len(scenes),3,3], and one
    sample per centre frame in scene order, `(scene index, [target path, reference paths at -d .. -1, +1 .. +d])`.  Scenes with
    fewer frames than sequence_length contribute no sample."""
    with open(os.path.join(root, "train.txt" if train else "val.txt")) as f:
        scenes = [line.rstrip("\n") for line in f if line.strip()]
    demi = (sequence_length - 1) // 2
    intrinsics = np.zeros((len(scenes), 3, 3), dtype=np.float32)
    samples = []
    for s, name in enumerate(scenes):
        folder = os.path.join(root, name)
        intrinsics[s] = np.loadtxt(os.path.join(folder, "cam.txt"), delimiter=",", dtype=np.float64).astype(np.float32).reshape(3, 3)
        imgs = sorted(os.path.join(folder, n) for n in os.listdir(folder)
                      if fnmatch.fnmatchcase(n, "*.jpg") and os.path.isfile(os.path.join(folder, n)))
        if len(imgs) < sequence_length:
            continue
        for i in range(demi, len(imgs) - demi):
            samples.append((s, [imgs[i]] + [imgs[i + j] for j in range(-demi, demi + 1) if j != 0]))
    return scenes, intrinsics, samples


def load_as_uint8(path):
    """One RGB JPEG -> uint8 [H,W,3]; ValueError for anything else (a greyscale frame, another format, not an image)."""
    from PIL import Image, UnidentifiedImageError
    try:
        with Image.open(path) as im:
            if im.format != "JPEG" or im.mode != "RGB":
                raise ValueError("%s: expected an RGB JPEG, found %s / %s" % (path, im.format, im.mode))
            return np.asarray(im)
    except UnidentifiedImageError as e:
        raise ValueError("%s: not an image (%s)" % (path, e))


def load_as_float(path):
    return load_as_uint8(path).astype(np.float32)


class SequenceFolder(data.Dataset):
    """root/scene_1/0000000.jpg, root/scene_1/0000001.jpg, .., root/scene_1/cam.txt, root/scene_2/0000000.jpg, ...
    transform: takes a list of images and the intrinsics matrix.  -> (tgt, refs, K, inv(K)) per sample, float32 HWC frames."""

    def __init__(self, root, seed=None, train=True, sequence_length=3, transform=None, target_transform=None):
        np.random.seed(seed)
        random.seed(seed)
        self.root = root
        self.scenes, intrinsics, found = crawl(root, train, sequence_length)
        self.samples = [{"intrinsics": intrinsics[s], "tgt": paths[0], "ref_imgs": paths[1:]} for s, paths in found]
        random.shuffle(self.samples)
        self.transform = transform

    def __getitem__(self, index):
        sample = self.samples[index]
        imgs = [load_as_float(p) for p in [sample["tgt"]] + sample["ref_imgs"]]
        intrinsics = np.copy(sample["intrinsics"])
        if self.transform is not None:
            imgs, intrinsics = self.transform(imgs, intrinsics)
        return imgs[0], imgs[1:], intrinsics, np.linalg.inv(intrinsics)

    def __len__(self):
        return len(self.samples)
