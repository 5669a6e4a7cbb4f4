"""ReferIt (saiapr_tc-12) datasets with the reference's names and semantics (dataset/Dataset_referit.py), on PIL only.

The reference composes torchvision's `Resize((size, size))`, `ToTensor()` and `Normalize(ImageNet)` on a PIL image; those are the
three steps dataset/transform.py already defines (`img.resize((s, s), BILINEAR)`, uint8 HWC -> float32 CHW / 255, (x - mean) / std),
so the image tensors here come through `normalize_table`, the table the HBM pipeline gathers through, and equal the reference's
bit for bit.  Targets are `cocomask.decode(rle).sum(axis=2).astype(uint8)`: a COUNT of covering segments, not a boolean
(Dataset_referit.py:141-144).  `tris_amd.dataset.hbm_referit` keeps the same items resident in HBM with the targets as run lengths.

ReferIt training is out of scope (the reference's train_stage1.py never constructs ImageLoader_train); the class is provided.
"""
import os
import pickle

import numpy as np
import torch
from PIL import Image

from ..CLIP import clip
from . import cocomask
from .transform import normalize_table


def pil_loader(path):
    with open(path, "rb") as f:
        img = Image.open(f)
        return img.convert("RGB")


def load_referit_gt_mask(mask_path):
    import scipy.io as sio          # (only this function needs scipy)
    mat = sio.loadmat(mask_path)
    return mat["segimg_t"] == 0


class FlickerTransform:
    """Resize((size, size)) + ToTensor + Normalize(ImageNet) of a PIL image (Dataset_referit.py:31-49) -> float32 [3,size,size]"""

    def __init__(self, size):
        self.size = int(size)
        self.lut = normalize_table()                                   # [3,256]

    def resize(self, img):
        """the uint8 [size,size,3] image behind the table: what the HBM cache keeps"""
        return np.asarray(img.resize((self.size, self.size), Image.BILINEAR))

    def __call__(self, img):
        a = torch.from_numpy(self.resize(img).copy()).to(torch.int64)  # [S,S,3]
        return torch.stack([self.lut[c][a[:, :, c]] for c in range(3)], 0)


def get_flicker_transform(args):
    """-> (transform_train, transform_test): the reference builds the same composition twice"""
    return FlickerTransform(args.size), FlickerTransform(args.size)


def _load_annotations(root, split):
    with open(os.path.join(root, "annotations", split + ".pickle"), "rb") as f:
        return pickle.load(f, encoding="latin1")


class ImageLoader_train(torch.utils.data.Dataset):
    def __init__(self, root, transform=None, split="train", loader=pil_loader, max_tokens=20, negative_samples=0, pseudo_path=None):
        self.annotations = _load_annotations(root, split)
        self.files = list(self.annotations.keys())
        self.transform, self.loader, self.split = transform, loader, split
        self.img_folder = os.path.join(root, "images")
        self.max_tokens, self.negative_samples, self.pseudo_path = max_tokens, negative_samples, pseudo_path
        self.all_refs = {}
        for key in self.files:                                          # refs flattened in file order
            for ref in self.annotations[str(key)]["annotations"]:
                self.all_refs[len(self.all_refs)] = ref

    def __getitem__(self, index):
        item = self.all_refs[index]
        img = Image.open(os.path.join(self.img_folder, str(item["image_id"]) + ".jpg")).convert("RGB")
        if self.transform is not None:
            img = self.transform(img)
        word_id = clip.tokenize(item["query"]).squeeze(0)[:self.max_tokens].numpy().copy()
        return img, word_id, -1

    def __len__(self):
        return len(self.all_refs)


def surviving(annotations, H, W):
    """indices of the annotations whose FIRST box covers strictly more than 5 % of the image (Dataset_referit.py:136)"""
    keep = []
    for i, a in enumerate(annotations):
        b = a["bbox"]
        if (b[0][3] - b[0][1]) * (b[0][2] - b[0][0]) > 0.05 * H * W:
            keep.append(i)
    return keep


class ImageLoader(torch.utils.data.Dataset):
    def __init__(self, root, transform=None, split="train", loader=pil_loader, max_tokens=20):
        self.annotations = _load_annotations(root, split)
        self.files = list(self.annotations.keys())
        self.transform, self.loader, self.split = transform, loader, split
        self.img_folder = os.path.join(root, "images")
        self.max_tokens = max_tokens

    def image_path(self, index):
        return os.path.join(self.img_folder, str(self.files[index]) + ".jpg")

    def __getitem__(self, index):
        item = str(self.files[index])
        img_path = self.image_path(index)
        img = Image.open(img_path).convert("RGB")
        image_sizes = (img.height, img.width)
        img = self.transform(img)
        ann = self.annotations[item]["annotations"]
        out = {}
        for i in surviving(ann, *image_sizes):                          # the keys keep the annotation's own index: gaps stay
            mask = cocomask.decode(ann[i]["segmentation"])
            out[str(i)] = {"sentences": ann[i]["query"],
                           "word_id": clip.tokenize(ann[i]["query"]).squeeze(0)[:self.max_tokens],
                           "bbox": np.array(ann[i]["bbox"]),
                           "mask": np.sum(mask, axis=2).astype(np.uint8)}
        return img, out, image_sizes, img_path

    def __len__(self):
        return len(self.files)


def get_refit_dataset(args):
    datadir = args.refer_data_root
    transform_train, transform_test = get_flicker_transform(args)
    ds_train = ImageLoader_train(datadir, split="train", transform=transform_train, max_tokens=args.max_query_len,
                                 negative_samples=args.negative_samples)
    ds_test = ImageLoader(datadir, split="test", transform=transform_test, max_tokens=args.max_query_len)
    return ds_train, ds_test
