"""HBM-resident input pipeline for Stage-1 (replaces DataLoader(ReferDataset, num_workers=2) +
dataset/transform.py for the training / evaluation loops).

At >800 img/s per GPU two CPU workers decoding and resizing JPEGs cannot feed the step, and an MI355X has 288 GB of
HBM: the whole dataset, decoded and resized ONCE to the network resolution, is a few GB of uint8 (RefCOCOg-umd train:
~21.9k images x 320*320*3 B = 6.7 GB).  So:

  build  (once):  PIL decode on the host -> uint8 to the GPU -> Pillow-exact antialiased resize (tris_resample_u8)
                  into images[n_img, S, S, 3];  masks -> Pillow-exact NEAREST (tris_gather2d_u8) into targets[n_ref, S, S]
                  (training) or kept at their original sizes in one flat buffer (evaluation);  token rows of every
                  sentence into tokens[n_sent, L].  Stage-2 training (`pseudo_path` set, not eval_mode): the [K,h,w] bool
                  stack of every ref's pseudo-mask file is uploaded as it is and summed + NEAREST-resized in one pass
                  (tris_mask_sum_nearest_u8) into pseudo[n_ref, S, S] -- ReferDataset.load_pseudo, once per run.
  batch  (per step):  the host draws the sentence / negatives of each sample with the reference's own
                  np.random.choice sequence (ReferDataset.sample_text), ships ONE small int64 index vector, and three
                  gather kernels assemble the batch: images are normalised through a 3x256 table straight into the
                  channels-last fp32 layout the stem convolution reads (no NCHW->NHWC pass).

Batches carry the reference's keys, shapes and dtypes (what default_collate makes of ReferDataset samples), so
train_one_epoch / validate take either loader.  A cache with `pseudo` adds targets["pseudo_gt"] (int64 [B,1,S,S]) to its
training batches, gathered by the same ref index vector as "target".

Evaluation datasets never read pseudo files, whatever their `pseudo_path`: the reference hands its evaluation datasets the
same directory (validate.py:64), their items carry no pseudo target, and files for those refs do not exist.

`cfg.poly_targets` (TRIS_POLY_TARGETS, default 0): the targets are built on the device from the annotation polygons
(dataset/poly_arena.py, csrc/polymask.hip) -- no ReferDataset.load_mask, no full-size mask upload; training rows are decoded at
the NEAREST resize's source positions, evaluation keeps the run ends and decodes a ref per batch.  Batches are bit-identical.

`images_from=`: a second cache over the same images at the same size (the train split evaluated after Stage-2 training)
takes the decoded and resized images of the first instead of decoding them again.
"""
import os

import numpy as np
import torch

from .. import ops
from ..config import cfg
from .transform import normalize_table


def _pseudo_file(ds, index):
    """the pseudo-mask file of training item `index` (dataset/ReferDataset.py:180); FileNotFoundError naming it if it is missing"""
    path = os.path.join(ds.pseudo_path, f"{index}_{ds.image_record(index)[1]}.npy")
    if not os.path.exists(path):
        raise FileNotFoundError(f"pseudo mask file {path} of training item {index} does not exist")
    return path


def _load_pseudo_stack(ds, index):
    """-> (the bool [K,h,w] instance masks of training item `index`, viewed as uint8; the file's path)"""
    path = _pseudo_file(ds, index)
    mask = np.asarray(np.load(path, allow_pickle=True).item()["mask"])
    if mask.dtype != np.bool_:
        raise TypeError(f"{path}: 'mask' is {mask.dtype}, expected bool (what make_ins_seg and IRNet write)")
    if mask.ndim != 3 or mask.shape[1] == 0 or mask.shape[2] == 0:
        raise ValueError(f"{path}: 'mask' has shape {mask.shape}, expected [K,h,w]")
    return np.ascontiguousarray(mask).view(np.uint8), path


class HbmReferCache:
    """images_from: another cache of the same size whose `images` are reused for every image id it holds.  When it holds all
    of them the tensor itself is shared; otherwise the missing ones are decoded and appended to a private tensor behind a
    device copy of the donor's.  Nothing else is shared."""

    def __init__(self, dataset, size, device="cuda", images_from=None):
        if not torch.cuda.is_available():
            raise ops.NoGpuError("HbmReferCache needs the GPU (the CPU path is DataLoader(ReferDataset))")
        self.dataset, self.size, self.device = dataset, size, torch.device(device)
        ds, S, dev = dataset, size, self.device
        n = len(ds)
        donor = images_from
        if donor is not None and (donor.size != S or donor.device != dev):
            raise ValueError(f"images_from: a cache of size {donor.size} on {donor.device} cannot serve size {S} on {dev}")
        slot = dict(donor.slot_by_img) if donor is not None else {}
        n_donor = len(slot)
        self.slot_of = np.empty(n, np.int64)
        recs = [ds.image_record(i) for i in range(n)]
        for i, (_, img_id, _) in enumerate(recs):
            self.slot_of[i] = slot.setdefault(img_id, len(slot))
        self.slot_by_img = slot           # image id -> row of `images`
        self.images_shared = donor is not None and len(slot) == n_donor
        if self.images_shared:
            self.images = donor.images
        else:
            self.images = torch.empty(len(slot), S, S, 3, dtype=torch.uint8, device=dev)
            if n_donor:
                self.images[:n_donor].copy_(donor.images)
        self.lut = normalize_table().to(dev)
        train = not ds.eval_mode
        self.targets = torch.empty(n, S, S, dtype=torch.uint8, device=dev) if train else None
        # Stage-2 pseudo targets: training items only (evaluation items carry none and have no files)
        with_pseudo = train and getattr(ds, "pseudo_path", None) is not None
        for i in range(n if with_pseudo else 0):
            _pseudo_file(ds, i)           # (a missing file stops the build here, before anything is decoded)
        self.pseudo = torch.empty(n, S, S, dtype=torch.uint8, device=dev) if with_pseudo else None
        self.eval_targets = []            # evaluation: masks at their original sizes
        boxes, paths, sizes, self.files = [], [], [], []
        # decode (once per image) and mask rasterisation (once per ref) on a few host threads -- Pillow releases the
        # GIL while decoding --, uploads and the resize kernels in order on this thread
        from concurrent.futures import ThreadPoolExecutor
        first_ref = {}
        for i in range(n):
            if self.slot_of[i] >= n_donor:      # (rows below n_donor are the donor's: already decoded)
                first_ref.setdefault(int(self.slot_of[i]), i)
        self.arena = None                 # cfg.poly_targets, evaluation: the refs' run ends (dataset/poly_arena.py: DeviceArena)
        poly = cfg.poly_targets
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            for s, img in zip(first_ref, pool.map(ds.load_image, first_ref.values())):
                ops.resample_u8(torch.from_numpy(np.asarray(img).copy()).to(dev), S, S, out=self.images[s])
            if poly:
                boxes, sizes, paths, self.files = self._poly_targets(recs)
            for i, (annot, bbox) in enumerate(pool.map(ds.load_mask, range(0 if poly else n))):
                m = torch.from_numpy(np.asarray(annot).copy()).to(dev)
                if train:
                    ops.resize_nearest_u8(m, S, S, out=self.targets[i])
                else:
                    self.eval_targets.append(m)
                w, h = annot.size
                fname = recs[i][2]["file_name"]
                boxes.append(bbox)
                sizes.append((h, w))
                paths.append(int(fname.split(".")[0].split("_")[-1]))
                self.files.append(fname)
            # (in chunks: a full-size [K,h,w] stack per ref is many times the cache row it becomes, so the readers must
            # not run a whole split ahead of the uploads)
            for a in range(0, n if with_pseudo else 0, 256):
                chunk = range(a, min(a + 256, n))
                for i, (stack, path) in zip(chunk, pool.map(lambda j: _load_pseudo_stack(ds, j), chunk)):
                    if stack.shape[0] > 255:
                        raise ValueError(f"{path}: {stack.shape[0]} masks, their sum does not fit the uint8 cache")
                    ops.mask_sum_nearest_u8(torch.from_numpy(stack).to(dev), S, S, out=self.pseudo[i])
        self.boxes = torch.from_numpy(np.stack(boxes).astype(np.int64)).to(dev)
        self.orig_size = torch.from_numpy(np.array(sizes, np.int64)).to(dev)
        self.img_path = torch.tensor(paths, dtype=torch.int64, device=dev).view(-1, 1)
        self._index_tokens(n)
        torch.cuda.synchronize(dev)

    def _poly_targets(self, recs):
        """cfg.poly_targets: the refs' polygons -> run ends on the device (dataset/poly_arena.py), once for the split; no
        ReferDataset.load_mask, no full-size mask.  Training: targets[i] decoded at the positions the NEAREST resize reads, the arena
        dropped afterwards.  Evaluation: the arena is kept and eval_batch decodes a ref when it is asked for.
        -> (boxes, sizes, paths, files) as load_mask and the build loop derive them from the annotation records"""
        from .poly_arena import PolyArena
        ds, S, refer = self.dataset, self.size, self.dataset.refer
        arena = PolyArena()
        boxes, sizes, paths, files = [], [], [], []
        for i in range(len(ds)):
            ref = refer.loadRefs(ds.ref_ids[i])[0]
            ann = refer.Anns[ref["ann_id"]]
            bbox = np.array(ann["bbox"], dtype=int)
            bbox[2], bbox[3] = bbox[0] + bbox[2], bbox[1] + bbox[3]
            image = refer.Imgs[ref["image_id"]]
            h, w = int(image["height"]), int(image["width"])
            arena.add_ref(ann["segmentation"], h, w, f"ref {ref['ref_id']} (annotation {ref['ann_id']})")
            fname = recs[i][2]["file_name"]
            boxes.append(bbox)
            sizes.append((h, w))
            paths.append(int(fname.split(".")[0].split("_")[-1]))
            files.append(fname)
        built = arena.build(self.device)
        if self.targets is not None:
            for i, ((lo, hi), (h, w)) in enumerate(zip(built.ranges.tolist(), sizes)):
                ops.rle_target_nearest(built, lo, hi, h, w, S, out=self.targets[i])
        else:
            self.arena, self.sizes_host = built, sizes
        return boxes, sizes, paths, files

    def _index_tokens(self, n):
        # token rows of every sentence, ref-major
        ds, dev = self.dataset, self.device
        self.sent_base = np.zeros(n + 1, np.int64)
        for i in range(n):
            self.sent_base[i + 1] = self.sent_base[i] + len(ds.input_ids[i])
        rows = torch.cat([r for ref in ds.input_ids for r in ref], dim=0)
        mrows = torch.cat([r for ref in ds.word_masks for r in ref], dim=0)
        assert rows.shape[1] * rows.element_size() % 4 == 0
        self.tokens = rows.contiguous().to(dev)
        self.token_masks = mrows.contiguous().to(dev)

    def nbytes(self):
        """device bytes this cache owns (images shared through images_from belong to the other cache)"""
        t = (0 if self.images_shared else self.images.numel()) + self.tokens.numel() * self.tokens.element_size()
        if self.targets is not None:
            t += self.targets.numel()
        if self.pseudo is not None:
            t += self.pseudo.numel()
        if self.arena is not None:    # (cfg.poly_targets: run ends instead of masks)
            t += self.arena.nbytes()
        return t + sum(m.numel() for m in self.eval_targets)


class HbmLoader:
    """Iterates (samples, targets) batches assembled on the GPU from an HbmReferCache.

    sampler: any iterable of dataset indices (e.g. torch DistributedSampler); otherwise sequential or shuffled with
    torch's global RNG like DataLoader(shuffle=True).  Evaluation datasets yield one ref per batch (all its sentences
    stacked on the last axis, the mask at its original size), as the reference's batch_size=1 loaders do."""

    def __init__(self, cache, batch_size=1, sampler=None, shuffle=False, drop_last=False, planar=False):
        self.cache, self.batch_size, self.sampler = cache, batch_size, sampler
        self.shuffle, self.drop_last, self.planar = shuffle, drop_last, planar
        self.dataset = cache.dataset
        if self.dataset.eval_mode and batch_size != 1:
            raise ValueError("evaluation refs have ragged sentence counts and mask sizes: batch_size must be 1")

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _order(self):
        if self.sampler is not None:
            return [int(i) for i in self.sampler]
        n = len(self.dataset)
        return torch.randperm(n).tolist() if self.shuffle else list(range(n))

    def __iter__(self):
        order = self._order()
        bs = self.batch_size
        for a in range(0, len(order), bs):
            chunk = order[a:a + bs]
            if len(chunk) < bs and self.drop_last:
                break
            yield self.eval_batch(chunk[0]) if self.dataset.eval_mode else self.train_batch(chunk)

    # ---- training: [B] refs, one drawn sentence + negatives each ---------------------------------------------------
    def train_batch(self, indices):
        c, ds = self.cache, self.dataset
        B, K = len(indices), ds.negative_samples
        picks = [ds.sample_text(i) for i in indices]          # host RNG, reference call order
        idx = np.empty(B * (3 + K), np.int64)
        idx[0:B] = indices
        idx[B:2 * B] = c.slot_of[indices]
        idx[2 * B:3 * B] = [c.sent_base[i] + p["choice"] for i, p in zip(indices, picks)]
        idx[3 * B:] = [c.sent_base[j] + s for p in picks for j, s in p["neg"]]
        dev = torch.from_numpy(idx).to(c.device, non_blocking=True)
        ref, slot, pos, neg = dev[0:B], dev[B:2 * B], dev[2 * B:3 * B], dev[3 * B:]
        S = c.size
        samples = {
            "img": ops.gather_normalize(c.images, slot, c.lut, planar=self.planar),
            "word_ids": ops.gather_rows(c.tokens, pos).unsqueeze(1),
            "word_masks": ops.gather_rows(c.token_masks, pos).unsqueeze(1),
        }
        if K > 0:
            samples["neg_sents"] = [tuple(ds.all_sentences[p["neg"][k][0]][p["neg"][k][1]] for p in picks) for k in range(K)]
            samples["neg_word_ids"] = ops.gather_rows(c.tokens, neg).view(B, K, -1)
        targets = {
            "target": ops.gather_rows(c.targets.view(-1, S * S), ref).view(B, 1, S, S).to(torch.int64),
            "img_path": ops.gather_rows(c.img_path, ref).view(B),
            "sentences": [ds.all_sentences[i][p["choice"]] for i, p in zip(indices, picks)],
            "boxes": ops.gather_rows(c.boxes, ref),
            "orig_size": ops.gather_rows(c.orig_size, ref),
            "img_path_full": [c.files[i] for i in indices],
        }
        if c.pseudo is not None:      # Stage-2 (ReferDataset.load_pseudo)
            targets["pseudo_gt"] = ops.gather_rows(c.pseudo.view(-1, S * S), ref).view(B, 1, S, S).to(torch.int64)
        return samples, targets

    # ---- evaluation: one ref, all its sentences ---------------------------------------------------------------------
    def eval_batch(self, index):
        c, ds = self.cache, self.dataset
        lo, hi = int(c.sent_base[index]), int(c.sent_base[index + 1])
        slot = torch.tensor([c.slot_of[index]], dtype=torch.int64, device=c.device)
        samples = {
            "img": ops.gather_normalize(c.images, slot, c.lut, planar=self.planar),
            "word_ids": c.tokens[lo:hi].t().unsqueeze(0).unsqueeze(0),        # [1, 1, L, S_ref]
            "word_masks": c.token_masks[lo:hi].t().unsqueeze(0).unsqueeze(0),
        }
        if c.arena is not None:       # cfg.poly_targets: the ref's mask from its run ends (pixels covered by exactly one polygon)
            a = c.arena
            m = ops.rle_decode_sum_arena(a.ends, a.seg_off, a.ranges[index:index + 1], *c.sizes_host[index])[0] == 1
        else:
            m = c.eval_targets[index]
        targets = {
            "target": m.view(1, 1, *m.shape).to(torch.int64),
            "img_path": c.img_path[index].view(1),
            "sentences": [(s,) for s in ds.all_sentences[index]],
            "boxes": c.boxes[index:index + 1],
            "orig_size": c.orig_size[index:index + 1],
            "img_path_full": [c.files[index]],
        }
        return samples, targets
