"""IRNet's training input pipeline on the MI355X: the reference's ReferAffinityDataset (IRNet/voc12/dataloader.py:191-285) and the
DataLoader of IRNet/step_refer/train_irn.py:18-28 / :86-91, fed from uint8 arenas in HBM through one kernel launch per batch
(csrc/irndata.hip).

    data = ReferAffinityData(train_list, label_dir, voc12_root, crop_size=512)       # the index: names, files, checks
    cache = HbmIrnCache(data, "cuda")                                                # every image and label decoded once, in HBM
    for img, label, label_reduced in IrnLoader(cache, batch_size=32, seed=0):        # device tensors
        trainer.train_step(img, label_reduced)
    trainer.fit_mean_shift(IrnLoader.top_left(cache, 32))                            # images only

The transform of one sample, in the reference's order (dataloader.py:222-261, IRNet/misc/imutils.py "imutils.py"):
  1. random_scale (imutils.py:48-55): s = lo + random() * (hi - lo); the target is (int(np.round(H s)), int(np.round(W s))); the image
     goes through Pillow's BICUBIC, the label through NEAREST (imutils.py:8-22).
  2. a grey image becomes three equal channels; (v / 255. - mean) / std per channel (dataloader.py:67-81).
  3. random_lr_flip (imutils.py:57-66): getrandbits(1).
  4. random_crop (imutils.py:68-114): randrange for the width, then the height; the image is pasted into zeros, the label into 255.
     The mean-shift pass (train_irn.py:86-89) draws nothing: scale 1, no flip, top_left_crop (imutils.py:116-130).
  5. the label at a quarter of the crop: pil_rescale(label, 0.25, 0) (dataloader.py:281).
The pair labels of GetAffinityLabelFromIndices (dataloader.py:83-109) are not built: the loss kernel derives them from the reduced
label (tris_amd.irn_loss).

Random numbers.  IrnLoader draws the epoch's order with torch.randperm under its own torch.Generator(seed), and every sample's
parameters from ONE random.Random(seed), in the order the samples are visited.  That is the sequence of the reference's
DataLoader with num_workers=0 under random.seed(seed); with worker processes the reference's own sequence depends on which worker
serves which batch and cannot be repeated, so only the single-process order is matched.

Only the host side lives here (tables, descriptors, checks); every pixel is the kernel's.  There is no CPU path.
"""
import json
import os
import random
from dataclasses import dataclass

import numpy as np

from . import pil_tables
from .._lib import CONSTS

TILE, PATCH, KMAX, ND = (CONSTS[k] for k in ("TRIS_IRN_AUG_TILE", "TRIS_IRN_AUG_PATCH", "TRIS_IRN_AUG_KMAX", "TRIS_IRN_AUG_DESC"))
# descriptor fields (csrc/irndata.hip)
(D_IMG, D_LAB, D_H, D_W, D_HT, D_WT, D_CT, D_CB, D_CL, D_CR, D_IT, D_IB, D_IL, D_IR, D_FLAGS, D_KH, D_KV, D_COLB, D_COLK, D_ROWB,
 D_ROWK, D_XNN, D_YNN) = range(23)
ARENA_SLACK = 16                     # spare bytes behind the last image: the kernel stages rows with aligned dword loads


def normalisation_table():
    """float32 [3, 256] as numpy: the IRNet pipeline's one table, irn_net.normalize_table (MEAN and STD live beside it)"""
    from ..irn_net import normalize_table
    return normalize_table().numpy()


# ------------------------------------------------------------------------------------------------------------------ the draw
@dataclass(frozen=True)
class IrnAugParams:
    """one sample's draw: scale, flip, the target size (Ht, Wt) and the box of get_random_crop_box (imutils.py:91):
    (cont_top, cont_bottom, cont_left, cont_right, img_top, img_bottom, img_left, img_right)"""
    scale: float
    flip: bool
    target: tuple
    box: tuple

    @staticmethod
    def target_size(H, W, scale):
        return int(np.round(H * scale)), int(np.round(W * scale))

    @classmethod
    def draw(cls, rng, H, W, crop_size, rescale=(0.5, 1.5), hor_flip=True):
        """the reference's calls on `rng` (a random.Random), in its order: random() -> scale; getrandbits(1) -> flip; randrange
        for the width, then the height, one call per axis in either branch of get_random_crop_box"""
        scale = 1.0
        if rescale:
            scale = rescale[0] + rng.random() * (rescale[1] - rescale[0])
        h, w = cls.target_size(H, W, scale)
        flip = bool(rng.getrandbits(1)) if hor_flip else False
        ch, cw = min(crop_size, h), min(crop_size, w)
        w_space, h_space = w - crop_size, h - crop_size
        if w_space > 0:
            cont_left, img_left = 0, rng.randrange(w_space + 1)
        else:
            cont_left, img_left = rng.randrange(-w_space + 1), 0
        if h_space > 0:
            cont_top, img_top = 0, rng.randrange(h_space + 1)
        else:
            cont_top, img_top = rng.randrange(-h_space + 1), 0
        return cls(scale, flip, (h, w), (cont_top, cont_top + ch, cont_left, cont_left + cw, img_top, img_top + ch, img_left,
                                         img_left + cw))

    @classmethod
    def top_left(cls, H, W, crop_size):
        """the mean-shift pass: no draws"""
        ch, cw = min(crop_size, H), min(crop_size, W)
        return cls(1.0, False, (H, W), (0, ch, 0, cw, 0, ch, 0, cw))

    @classmethod
    def explicit(cls, H, W, crop_size, scale, flip, top, left):
        """for tests: `top` / `left` is the one free offset of its axis -- the container's when the target fits the crop, the
        image's otherwise"""
        h, w = cls.target_size(H, W, scale)
        ch, cw = min(crop_size, h), min(crop_size, w)
        ct, it = (0, top) if h > crop_size else (top, 0)
        cl, il = (0, left) if w > crop_size else (left, 0)
        return cls(float(scale), bool(flip), (h, w), (ct, ct + ch, cl, cl + cw, it, it + ch, il, il + cw))


# ---------------------------------------------------------------------------------------------------------------- the index
def check_crop_size(crop_size):
    if crop_size <= 0 or crop_size % 4 != 0:
        raise ValueError(f"crop_size {crop_size} is not a positive multiple of 4: the reduced label and the reference's PathIndex "
                         "are crop_size // 4 wide")


class ReferAffinityData:
    """the index of the reference's ReferAffinityDataset: names from the JSON list, the image of a name by make_ins_seg's rule,
    its label at {label_dir}/{name}.png"""

    def __init__(self, train_list, label_dir, voc12_root, crop_size, rescale=(0.5, 1.5), hor_flip=True, crop_method="random"):
        check_crop_size(crop_size)
        if crop_method not in ("random", "top_left"):
            raise ValueError(f"crop_method {crop_method!r}: 'random' or 'top_left'")
        with open(train_list) as f:
            self.names = list(json.load(f))
        self.label_dir, self.voc12_root, self.crop_size = label_dir, voc12_root, int(crop_size)
        self.rescale, self.hor_flip, self.crop_method = (tuple(rescale) if rescale else None), bool(hor_flip), crop_method

    def __len__(self):
        return len(self.names)

    def image_id(self, i):
        from ..make_ins_seg import image_id
        return image_id(self.names[i])

    def image_path(self, i):
        from ..make_ins_seg import image_file
        return image_file(self.names[i], self.voc12_root)

    def label_path(self, i):
        return os.path.join(self.label_dir, self.names[i] + ".png")

    def load_image(self, i):
        """uint8 [H,W,3]; a grey image becomes three equal channels (its bicubic resize is the same in each)"""
        from ..make_ins_seg import load_image
        return load_image(self.image_path(i))

    def load_label(self, i, size=None):
        """uint8 [H,W]; a missing file, or one that is not the image's size, is an error that names the file"""
        from PIL import Image
        path = self.label_path(i)
        if not os.path.exists(path):
            raise FileNotFoundError(f"label file {path} of {self.names[i]!r} is missing")
        with Image.open(path) as im:
            a = np.asarray(im)
        if a.ndim != 2 or a.dtype != np.uint8:
            raise ValueError(f"label file {path}: expected an 8-bit single-channel image, got {a.shape} {a.dtype}")
        if size is not None and tuple(a.shape) != tuple(size):
            raise ValueError(f"label file {path} is {a.shape[0]}x{a.shape[1]}, its image {self.image_path(i)} is {size[0]}x{size[1]}")
        return np.ascontiguousarray(a)

    def params(self, rng, H, W):
        if self.crop_method == "top_left":
            return IrnAugParams.top_left(H, W, self.crop_size)
        return IrnAugParams.draw(rng, H, W, self.crop_size, self.rescale, self.hor_flip)


# ------------------------------------------------------------------------------------------------------------ table builder
def axis_entries(in_size, out_size, first, count, reverse=False):
    """the resized indices the crop window needs along one axis, in the window's order: first .. first + count - 1, or mirrored
    (the horizontal flip: column x of the flipped image is column out_size - 1 - x)"""
    idx = np.arange(first, first + count, dtype=np.int64)
    return (out_size - 1 - idx) if reverse else idx


def build_batch(samples, params, crop_size):
    """samples: [(image offset, label offset, H, W)] of the arenas; params: [IrnAugParams] -> (desc int64 [B, ND], tables int32 [n]).
    Only the window's entries are built: at most crop_size columns and rows per sample.  An axis whose size does not change has
    no table (Pillow skips that pass); the label's source indices are always there (NEAREST at an unchanged size is the identity)."""
    check_crop_size(crop_size)
    B = len(samples)
    desc = np.zeros((B, ND), np.int64)
    entries, axes, slots = [], [], []
    for b, ((img_off, lab_off, H, W), p) in enumerate(zip(samples, params)):
        Ht, Wt = p.target
        ct, cb, cl, cr, it, ib, il, ir = p.box
        cols = axis_entries(W, Wt, il, ir - il, p.flip)
        rows = axis_entries(H, Ht, it, ib - it)
        for name, idx, size in (("column", cols, Wt), ("row", rows, Ht)):
            if idx.size and (idx.min() < 0 or idx.max() >= size):
                raise ValueError(f"sample {b}: the box's image {name}s reach outside the resized image ({size} {name}s)")
        entries.append((cols, rows))
        if Wt != W:
            axes.append((W, Wt, cols))
            slots.append((b, D_COLB, D_COLK, D_KH, 1))
        if Ht != H:
            axes.append((H, Ht, rows))
            slots.append((b, D_ROWB, D_ROWK, D_KV, 2))
    parts, n = [], 0

    def put(a):
        nonlocal n
        a = np.ascontiguousarray(a, np.int32).reshape(-1)
        off = n
        parts.append(a)
        n += a.size
        return off

    for (b, o_b, o_k, o_n, flag), (bounds, kk, ks) in zip(slots, pil_tables.resample_taps_many(axes, "bicubic")):
        desc[b, o_b], desc[b, o_k], desc[b, o_n] = put(bounds), put(kk), ks
        desc[b, D_FLAGS] |= flag
    for b, ((img_off, lab_off, H, W), p) in enumerate(zip(samples, params)):
        d = desc[b]
        d[[D_IMG, D_LAB, D_H, D_W, D_HT, D_WT]] = (img_off, lab_off, H, W) + tuple(p.target)
        d[D_CT:D_IR + 1] = p.box
        d[D_XNN] = put(pil_tables.nearest_taps(W, p.target[1], entries[b][0]))
        d[D_YNN] = put(pil_tables.nearest_taps(H, p.target[0], entries[b][1]))
        if p.flip:
            d[D_FLAGS] |= 4
    tables = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    return desc, tables


def _window_extent(first, end):
    """the most source indices any TILE consecutive entries reach (the entries are monotone, either way)"""
    if first.size == 0:
        return 0
    if first.size > 1 and first[0] > first[-1]:
        first, end = first[::-1], end[::-1]
    hi = np.minimum(np.arange(first.size) + TILE - 1, first.size - 1)
    return int((end[hi] - first).max())


def validate_batch(desc, tables, crop_size, img_bytes, lab_bytes):
    """refuse, by name, whatever would make the kernel read or write outside its buffers: a box outside the crop, a table entry
    outside its image, more taps or a wider source patch than the kernel's tile holds, an image outside its arena.
    img_bytes: the image arena's size without its ARENA_SLACK."""
    check_crop_size(crop_size)
    desc = np.asarray(desc, np.int64)
    tables = np.asarray(tables, np.int32)
    if desc.ndim != 2 or desc.shape[1] != ND:
        raise ValueError(f"descriptors: expected [B, {ND}], got {desc.shape}")
    for b, d in enumerate(desc):
        H, W, Ht, Wt = (int(d[k]) for k in (D_H, D_W, D_HT, D_WT))
        ct, cb, cl, cr, it, ib, il, ir = (int(v) for v in d[D_CT:D_IR + 1])
        if min(H, W, Ht, Wt) <= 0:
            raise ValueError(f"sample {b}: empty image or target ({H}x{W} -> {Ht}x{Wt})")
        if d[D_IMG] < 0 or d[D_IMG] % 16 or d[D_IMG] + H * W * 3 > img_bytes:
            raise ValueError(f"sample {b}: image offset {d[D_IMG]} ({H}x{W}x3) is outside the image arena or not 16-byte aligned")
        if d[D_LAB] < 0 or d[D_LAB] + H * W > lab_bytes:
            raise ValueError(f"sample {b}: label offset {d[D_LAB]} ({H}x{W}) is outside the label arena")
        if not (0 <= ct < cb <= crop_size and 0 <= cl < cr <= crop_size):
            raise ValueError(f"sample {b}: box rows {ct}:{cb}, columns {cl}:{cr} outside the crop of {crop_size}")
        if cb - ct != ib - it or cr - cl != ir - il or not (0 <= it < ib <= Ht and 0 <= il < ir <= Wt):
            raise ValueError(f"sample {b}: image box rows {it}:{ib}, columns {il}:{ir} does not fit the target {Ht}x{Wt} "
                             f"or the box {cb - ct}x{cr - cl}")
        flags = int(d[D_FLAGS])
        if bool(flags & 1) != (Wt != W) or bool(flags & 2) != (Ht != H):
            raise ValueError(f"sample {b}: table flags {flags} do not go with {H}x{W} -> {Ht}x{Wt}")
        for axis, n, size, has, o_b, o_k, ks, o_nn, lo in (("column", cr - cl, W, flags & 1, D_COLB, D_COLK, D_KH, D_XNN, il),
                                                          ("row", ib - it, H, flags & 2, D_ROWB, D_ROWK, D_KV, D_YNN, it)):
            def span(off, count, what):
                if off < 0 or off + count > tables.size:
                    raise ValueError(f"sample {b}: {axis} {what} at {off}+{count} outside the packed tables ({tables.size})")
                return tables[off:off + count]
            nn = span(int(d[o_nn]), n, "label indices")
            if nn.max() >= size or nn.min() < -1:
                raise ValueError(f"sample {b}: a label {axis} index reads outside its image ({size} {axis}s)")
            if has:
                k = int(d[ks])
                if not 1 <= k <= KMAX:
                    raise ValueError(f"sample {b}: {k} taps per {axis} (the kernel holds {KMAX}): scale too small")
                bounds = span(int(d[o_b]), 2 * n, "bounds").reshape(n, 2).astype(np.int64)
                span(int(d[o_k]), k * n, "taps")
                first, end = bounds[:, 0], bounds[:, 0] + bounds[:, 1]
                if first.min() < 0 or end.max() > size or bounds[:, 1].min() < 1 or bounds[:, 1].max() > k:
                    raise ValueError(f"sample {b}: a {axis} tap reads outside its image ({size} {axis}s) or its table row")
            else:   # no pass along this axis: entry e reads lo + e (mirrored under the flip), inside the target by the box check
                first = np.arange(lo, lo + n, dtype=np.int64)
                if axis == "column" and flags & 4:
                    first = Wt - 1 - first
                end = first + 1
            step = np.diff(first)
            if step.size and step.min() < 0 and step.max() > 0:
                raise ValueError(f"sample {b}: {axis} entries are not monotone")
            if _window_extent(first, end) > PATCH:
                raise ValueError(f"sample {b}: one tile's {axis} taps reach {_window_extent(first, end)} source {axis}s "
                                 f"(the kernel stages {PATCH}): scale too small")


def pack_arena(arrays, align=16, slack=0):
    """[uint8 arrays] -> (uint8 arena, offsets), every offset a multiple of `align`, `slack` spare bytes at the end"""
    offsets, n = [], 0
    for a in arrays:
        offsets.append(n)
        n += -(-a.size // align) * align
    arena = np.zeros(n + slack, np.uint8)
    for a, o in zip(arrays, offsets):
        arena[o:o + a.size] = np.ascontiguousarray(a, np.uint8).reshape(-1)
    return arena, offsets


# ---------------------------------------------------------------------------------------------------------- cache and loader
class HbmIrnCache:
    """every distinct image of the list decoded once (the list is per referring expression: ids repeat), every label once, packed
    into two uint8 arenas on `device` at 16-byte-aligned offsets.  images_from: a mapping image id -> decoded uint8 [H,W,3] or
    [H,W] array, used instead of the files for the ids it holds."""

    def __init__(self, data, device="cuda", images_from=None):
        import torch
        from .. import ops
        if not torch.cuda.is_available() or torch.device(device).type != "cuda":
            raise ops.NoGpuError("tris_amd.dataset.irn_data keeps its arenas on MI355X only; there is no CPU fallback")
        self.data, self.device = data, torch.device(device)
        images, slot, self.image_slot, labels = [], {}, [], []
        for i in range(len(data)):
            key = data.image_id(i)
            if key not in slot:
                if images_from is not None and key in images_from:
                    a = np.asarray(images_from[key], np.uint8)
                    a = np.stack([a, a, a], axis=2) if a.ndim == 2 else a
                else:
                    a = data.load_image(i)
                if a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError(f"image {key}: expected [H,W,3] or [H,W], got {a.shape}")
                slot[key] = len(images)
                images.append(np.ascontiguousarray(a))
            self.image_slot.append(slot[key])
            labels.append(data.load_label(i, images[slot[key]].shape[:2]))
        img_arena, self.image_offsets = pack_arena(images, 16, ARENA_SLACK)
        lab_arena, self.label_offsets = pack_arena(labels, 16)
        self.image_sizes = [a.shape[:2] for a in images]
        self.img_arena = torch.from_numpy(img_arena).to(self.device)
        self.lab_arena = torch.from_numpy(lab_arena).to(self.device)
        self.lut = torch.from_numpy(normalisation_table()).to(self.device)

    def __len__(self):
        return len(self.data)

    def size(self, i):
        return self.image_sizes[self.image_slot[i]]

    def sample(self, i):
        """(image offset, label offset, H, W) of name i"""
        H, W = self.size(i)
        return self.image_offsets[self.image_slot[i]], self.label_offsets[i], H, W

    @property
    def nbytes(self):
        return self.img_arena.numel() + self.lab_arena.numel()


class IrnLoader:
    """batches (img float32 [B,3,crop,crop] in channels-last memory, label uint8 [B,crop,crop], label_reduced uint8
    [B,crop/4,crop/4]) on the cache's device; the random numbers are the module docstring's."""
    RING = 4        # pinned staging buffers in flight: a buffer is reused only after its copy has been done

    def __init__(self, cache, batch_size, seed=0, shuffle=True, drop_last=True, images_only=False):
        import torch
        self.cache, self.batch_size, self.shuffle, self.drop_last = cache, int(batch_size), bool(shuffle), bool(drop_last)
        self.images_only = bool(images_only)
        self.generator = torch.Generator().manual_seed(int(seed))
        self.rng = random.Random(seed)
        self._ring, self._turn, self._dev = [[None, None] for _ in range(self.RING)], 0, None   # [pinned buffer, copy event]
        self._top_left = False

    @classmethod
    def top_left(cls, cache, batch_size):
        """the mean-shift pass's iterator (train_irn.py:86-91): in list order, no draws, incomplete batches dropped; images only"""
        it = cls(cache, batch_size, shuffle=False, drop_last=True, images_only=True)
        it._top_left = True
        return it

    def __len__(self):
        n = len(self.cache)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def order(self):
        """this epoch's order: torch.randperm under the loader's generator (advances it)"""
        import torch
        n = len(self.cache)
        return torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))

    def draw(self, indices):
        data = self.cache.data
        if self._top_left:
            return [IrnAugParams.top_left(*self.cache.size(i), data.crop_size) for i in indices]
        return [data.params(self.rng, *self.cache.size(i)) for i in indices]

    def __iter__(self):
        order = self.order()
        for k in range(len(self)):
            indices = order[k * self.batch_size:(k + 1) * self.batch_size]
            out = self.augment(indices, self.draw(indices))
            yield out[0] if self.images_only else out

    def _staging(self, nbytes):
        import torch
        slot = self._ring[self._turn % self.RING]
        self._turn += 1
        if slot[1] is not None:
            slot[1].synchronize()       # (the copy of RING batches ago: long done unless the host runs that far ahead)
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
        if self._dev is None or self._dev.numel() < nbytes:
            self._dev = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=self.cache.device)
        return slot

    def prepare(self, indices, params):
        """the host side of one batch: tables, descriptors, checks, and their one copy to the device (queued, not waited for)
        -> (device buffer, descriptor bytes): what the launch takes.  The buffer is the loader's own and holds until the next call."""
        import torch
        cache, crop = self.cache, self.cache.data.crop_size
        desc, tables = build_batch([cache.sample(i) for i in indices], params, crop)
        validate_batch(desc, tables, crop, cache.img_arena.numel() - ARENA_SLACK, cache.lab_arena.numel())
        nd, nt = desc.size * 8, tables.size * 4
        slot = self._staging(nd + nt)
        host = slot[0].numpy()
        host[:nd] = desc.reshape(-1).view(np.uint8)
        host[nd:nd + nt] = tables.view(np.uint8)
        with torch.cuda.device(cache.device):
            self._dev[:nd + nt].copy_(slot[0][:nd + nt], non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
        return self._dev, nd

    def augment(self, indices, params):
        """one batch with explicit parameters -> (img, label, label_reduced).  Descriptors and tables travel in one pinned buffer
        and one copy; one kernel launch; no device-to-host sync."""
        import torch
        from .. import ops
        cache = self.cache
        packed, nd = self.prepare(indices, params)
        with torch.cuda.device(cache.device):
            return ops.irn_augment_batch(cache.img_arena, cache.lab_arena, packed, nd, cache.lut, len(indices), cache.data.crop_size)
