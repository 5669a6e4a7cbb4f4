"""HBM-resident ReferIt evaluation set (sibling of dataset/hbm.py; replaces DataLoader(ImageLoader, batch_size=1) for
tris_amd.validate_referit).

  build (once):  every image PIL-decoded on a few host threads, uploaded and resized by ops.resample_u8 (Pillow's BILINEAR) into
                 images uint8 [N,S,S,3];  per image (H, W), and for the sentences that pass the dataset's 5 % rule their token
                 rows, boxes and segment ranges into ONE run-boundary arena (dataset/rle_arena.py).  The test split's targets
                 are ~10 k images x several sentences at the images' own sizes: tens of GB dense, a few MB as run lengths.
  per image:     gather_normalize of its row (ToTensor + Normalize through the 3x256 table) and a DeviceGroup;
                 the targets are decoded on the device by the evaluation loop (ops.rle_decode_sum_arena) and never leave it.

A missing image or a malformed RLE stops the build, naming the file or the key.
"""
import os

import numpy as np
import torch

from .. import ops
from ..CLIP import clip
from .Dataset_referit import surviving
from .rle_arena import RleArena
from .transform import normalize_table


class DeviceGroup:
    """what HbmReferitLoader hands tris_amd.validate_referit in place of the DataLoader's dict of sentences: the K surviving
    sentences of one image with their targets as segment ranges into the device arena"""

    def __init__(self, keys, word_ids, bboxes, ranges, ends, seg_off):
        self.keys, self.word_ids, self.bboxes = keys, word_ids, bboxes         # [K] str, int64 [K,L] device, K x int array [n,4]
        self.ranges, self.ends, self.seg_off = ranges, ends, seg_off           # int32 [K,2], the arena

    def __len__(self):
        return len(self.keys)


class HbmReferitCache:
    def __init__(self, dataset, size, device="cuda"):
        if not torch.cuda.is_available():
            raise ops.NoGpuError("HbmReferitCache needs the GPU (the CPU path is DataLoader(ImageLoader))")
        self.dataset, self.size, self.device = dataset, int(size), torch.device(device)
        ds, S, dev = dataset, self.size, self.device
        n = len(ds)
        paths = [ds.image_path(i) for i in range(n)]
        for p in paths:
            if not os.path.isfile(p):
                raise FileNotFoundError(f"image {p} of the {ds.split} split does not exist")
        self.paths = paths
        self.images = torch.empty(n, S, S, 3, dtype=torch.uint8, device=dev)
        self.lut = normalize_table().to(dev)
        self.sizes = []
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            for i, img in enumerate(pool.map(ds.loader, paths)):
                self.sizes.append((img.height, img.width))
                ops.resample_u8(torch.from_numpy(np.asarray(img).copy()).to(dev), S, S, out=self.images[i])
        arena = RleArena()
        self.keys, self.bboxes, self.sentences, self.sent_base = [], [], [], np.zeros(n + 1, np.int64)
        rows, ranges = [], []
        for i in range(n):
            key = str(ds.files[i])
            ann = ds.annotations[key]["annotations"]
            H, W = self.sizes[i]
            keep = surviving(ann, H, W)
            for j in keep:
                ranges.append(arena.add_sentence(ann[j]["segmentation"], H, W, f"{key} annotation {j}"))
                rows.append(clip.tokenize(ann[j]["query"]).squeeze(0)[:ds.max_tokens])
            self.keys.append([str(j) for j in keep])
            self.bboxes.append([np.array(ann[j]["bbox"]).reshape(-1, 4) for j in keep])
            self.sentences.append([ann[j]["query"] for j in keep])
            self.sent_base[i + 1] = self.sent_base[i] + len(keep)
        L = ds.max_tokens
        self.tokens = (torch.stack(rows) if rows else torch.zeros(0, L)).to(torch.int64).to(dev)
        self.ranges = torch.tensor(ranges, dtype=torch.int32).reshape(-1, 2).to(dev)
        self.ends, self.seg_off = arena.to(dev)
        torch.cuda.synchronize(dev)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.images, self.tokens, self.ranges, self.ends, self.seg_off))


class HbmReferitLoader:
    """yields (img [1,3,S,S], DeviceGroup, (H, W), [img_path]) per image, in file order: the items of
    DataLoader(ImageLoader, batch_size=1) with everything already on the device"""

    def __init__(self, cache):
        self.cache, self.dataset = cache, cache.dataset

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        c = self.cache
        for i in range(len(self)):
            lo, hi = int(c.sent_base[i]), int(c.sent_base[i + 1])
            slot = torch.tensor([i], dtype=torch.int64, device=c.device)
            img = ops.gather_normalize(c.images, slot, c.lut) if hi > lo else None     # (an image without sentences is not read)
            yield img, DeviceGroup(c.keys[i], c.tokens[lo:hi], c.bboxes[i], c.ranges[lo:hi], c.ends, c.seg_off), c.sizes[i], \
                [c.paths[i]]
