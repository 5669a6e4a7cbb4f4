"""How good are the artefacts between Stage 1 and Stage 2?  Response maps, CRF labels and instance masks scored against the REFER
ground truth of their refs (csrc/labelscore.hip; the command line is tris_amd.eval_pseudo).

The reference names such passes (IRNet/run_sample_refer.py:59 --cam_eval_thres, :98 --eval_cam_pass, :102 --eval_ins_seg_pass) and
ships none of them, so the metrics below are this project's definitions.  They are pinned to tris_amd.validate's I/U rule
(validate.py:183-190: pred = map > threshold, I = sum(pred & target), U = sum(pred | target), iou = I/U, 0 when U is 0) and to the
host rasteriser (ReferDataset.load_mask: the pixels covered by exactly one polygon), not to a recording.

The ground truth of every ref the name list mentions is built once as run ends on the device (dataset/poly_arena.py) and read there
by the scoring kernels: no ref is rasterised on the host and no full-size target is formed.

A name is `{idx}_{img_id}` (what validate_same_sentence(save_cam=True) lists with PRMS) or `{idx}_{j}_{img_id}` (without): idx, the
first field, is the item index of the split's dataset, and the last field is the image id, as make_ins_seg.image_id reads it.

Three artefacts, three on-disk formats:
  score_cams    D/{name}.npy  float32 [H,W]                     -> int64 [N, T+1, 2]   per name: bin of the value x ground-truth bit
  score_labels  L/{name}.png  8-bit grey, 1 / 0 / 255           -> int64 [N, 3, 2]     rows: label 0, label 1, label 255
  score_masks   O/{name}.npy  dict with 'mask' bool [K,h,w]     -> int64 [N, 3, 2], K  rows: sum 0, sum 1, sum > 1
  score_instances  the same file with its 'score' [K]           -> per name int64 [K+3, 2]   rows: sum 0, 1, > 1, then one per
                   instance; optionally on the size x size grid Stage 2 trains on (ops.score_planes; summarise_instances: top-1 /
                   best / scored / union IoU, the score-0 fragments' share of the false positives, AP by the VOC rule)
Files are read ahead on a few host threads; consecutive names of one image share a launch pair of the map kernels (at most
GROUP_MAX); the histograms stay on the device until a pass ends (or FLUSH names have gathered), so the host waits for the device
less often than once per group.  The summarise_* functions are pure numpy.
"""
import os
from collections import deque

import numpy as np

GROUP_MAX = 64             # maps of one image scored by one launch pair
FLUSH = 4096               # names whose histograms may wait on the device
READ_AHEAD = 128           # files in flight in front of the scoring loop
VALIDATE_THRESHOLD = 1e-9  # tris_amd.validate's own (validate.py:186)


def default_thresholds():
    """validate's threshold, then 0.05 .. 0.95 in steps of 0.05"""
    return [VALIDATE_THRESHOLD] + [round(0.05 * k, 2) for k in range(1, 20)]


# ------------------------------------------------------------------------------------------------------------------ names
def parse_name(name):
    """'{idx}_{img_id}' or '{idx}_{j}_{img_id}' -> (idx, image-id field); ValueError naming the name"""
    fields = str(name).split("_")
    if len(fields) not in (2, 3) or not all(f.isdigit() for f in fields):
        raise ValueError(f"name {name!r} is neither '{{idx}}_{{img_id}}' nor '{{idx}}_{{j}}_{{img_id}}'")
    return int(fields[0]), fields[-1]


def resolve_names(names, dataset):
    """the item index of every name, checked against the dataset: an index outside it, or a last field that is not that item's
    image id, is a ValueError naming the name"""
    out = []
    for name in names:
        idx, img = parse_name(name)
        if not 0 <= idx < len(dataset):
            raise ValueError(f"name {name!r}: item index {idx} lies outside the split's {len(dataset)} items")
        want = dataset.image_record(idx)[1]
        if img != str(want):
            raise ValueError(f"name {name!r}: its last field {img} is not the image id {want} of item {idx}")
        out.append(idx)
    return out


class GroundTruth:
    """One PolyArena (dataset/poly_arena.py) for the refs `indices` mentions, built on the device once.  `refs[idx]` =
    (lo, hi, h, w, img_id): the ref's segments in the arena, its image's size and id.  The polygons are refer.Anns[...]['segmentation'],
    taken exactly as HbmReferCache._poly_targets takes them."""

    def __init__(self, dataset, indices, device="cuda"):
        from .dataset.poly_arena import PolyArena
        self.dataset, self.refs = dataset, {}
        refer, arena = dataset.refer, PolyArena()
        for idx in indices:
            idx = int(idx)
            if idx in self.refs:
                continue
            if not 0 <= idx < len(dataset):
                raise ValueError(f"item index {idx} lies outside the split's {len(dataset)} items")
            ref = refer.loadRefs(dataset.ref_ids[idx])[0]
            ann = refer.Anns[ref["ann_id"]]
            image = refer.Imgs[ref["image_id"]]
            h, w = int(image["height"]), int(image["width"])
            lo, hi = arena.add_ref(ann["segmentation"], h, w, f"ref {ref['ref_id']} (annotation {ref['ann_id']})")
            self.refs[idx] = (lo, hi, h, w, ref["image_id"])
        self.arena = arena.build(device)          # (NoGpuError without a GPU)
        self.device = self.arena.ends.device

    def of_names(self, names):
        """-> per name its (lo, hi, h, w, img_id); the names are checked as resolve_names checks them"""
        return [self.refs[i] for i in resolve_names(names, self.dataset)]


# ------------------------------------------------------------------------------------------------------------------ readers
def _need(path, what):
    if not os.path.exists(path):
        raise FileNotFoundError(f"{what} {path} does not exist")


def _read_cam(path, h, w):
    _need(path, "response map")
    cam = np.load(path, allow_pickle=True)
    if not isinstance(cam, np.ndarray) or cam.dtype == object or cam.ndim != 2:
        raise ValueError(f"{path}: expected a response map [H,W], got {getattr(cam, 'shape', type(cam).__name__)}")
    if cam.shape != (h, w):
        raise ValueError(f"{path}: response map {cam.shape[0]}x{cam.shape[1]} does not go with an image of {h}x{w}")
    return np.ascontiguousarray(cam, np.float32)


def _read_label(path, h, w):
    from PIL import Image
    _need(path, "label file")
    with Image.open(path) as im:
        if im.mode != "L":
            raise ValueError(f"{path}: image mode {im.mode}, expected 8-bit grey ('L')")
        lab = np.asarray(im).copy()
    if lab.shape != (h, w):
        raise ValueError(f"{path}: label {lab.shape[0]}x{lab.shape[1]} does not go with an image of {h}x{w}")
    seen = np.bincount(lab.reshape(-1), minlength=256)
    seen[[0, 1, 255]] = 0
    if seen.any():
        raise ValueError(f"{path}: label value {int(np.nonzero(seen)[0][0])}, expected 1 (object), 0 (background) or 255 (neither)")
    return lab


def _read_masks(path, h, w):
    _need(path, "instance-mask file")
    rec = np.load(path, allow_pickle=True)
    rec = rec.item() if isinstance(rec, np.ndarray) and rec.dtype == object and rec.ndim == 0 else rec
    if not isinstance(rec, dict) or "mask" not in rec:
        raise ValueError(f"{path}: expected a pickled dict with 'mask'")
    mask = np.asarray(rec["mask"])
    if mask.dtype != np.bool_:
        raise TypeError(f"{path}: 'mask' is {mask.dtype}, expected bool (what make_ins_seg and IRNet write)")
    if mask.shape[0:1] == (0,):
        return np.zeros((0, h, w), np.uint8)
    if mask.ndim != 3:
        raise ValueError(f"{path}: 'mask' has shape {mask.shape}, expected [K,h,w]")
    if mask.shape[1:] != (h, w):
        raise ValueError(f"{path}: masks {mask.shape[1]}x{mask.shape[2]} do not go with an image of {h}x{w}")
    if mask.shape[0] > 255:
        raise ValueError(f"{path}: {mask.shape[0]} masks, their sum does not fit a byte (at most 255)")
    return np.ascontiguousarray(mask).view(np.uint8)


def _read_instances(path, h, w):
    """_read_masks and the file's 'score' as float64 [K]: make_ins_seg writes one per instance (0 for a fragment under 1 % of the
    image, IRNet/step_refer/make_ins_seg_labels.py:95-101; int64 zeros where nothing was found), so integer and float dtypes both
    pass; a missing, mis-sized or non-finite 'score' is a ValueError naming the file"""
    stack = _read_masks(path, h, w)                    # (its checks as they are; the dict is unpickled once more for the scores)
    rec = np.load(path, allow_pickle=True).item()
    if "score" not in rec:
        raise ValueError(f"{path}: the dict has no 'score' (one per instance, as make_ins_seg writes it)")
    score = np.asarray(rec["score"])
    if score.dtype.kind not in "iuf" or score.shape != (stack.shape[0],):
        raise ValueError(f"{path}: 'score' is {score.dtype} {tuple(score.shape)}, expected one number for each of the "
                         f"{stack.shape[0]} masks")
    score = score.astype(np.float64)
    if not np.isfinite(score).all():
        raise ValueError(f"{path}: 'score' holds a non-finite value ({score[~np.isfinite(score)][0]}) at instance "
                         f"{int(np.nonzero(~np.isfinite(score))[0][0])}")
    return stack, score


def _read_ahead(fn, jobs):
    """fn(*job) for every job, in order, READ_AHEAD of them in flight on min(16, cpu_count) threads"""
    from concurrent.futures import ThreadPoolExecutor
    jobs = iter(jobs)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        pending = deque()
        try:
            for job in jobs:
                pending.append(pool.submit(fn, *job))
                if len(pending) >= READ_AHEAD:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()
        finally:
            for f in pending:
                f.cancel()


def _groups(recs):
    """consecutive names of one image -> [start, stop) slices of at most GROUP_MAX names"""
    a = 0
    for k in range(1, len(recs) + 1):
        if k == len(recs) or recs[k][4] != recs[a][4] or k - a == GROUP_MAX:
            yield a, k
            a = k


class _Gather:
    """device histograms waiting for one copy to the host"""

    def __init__(self, shape):
        self.shape, self.dev, self.host, self.waiting = shape, [], [], 0

    def add(self, t):
        self.dev.append(t.reshape((-1,) + self.shape))
        self.waiting += self.dev[-1].shape[0]
        if self.waiting >= FLUSH:
            self.flush()

    def flush(self):
        import torch
        if self.dev:
            self.host.append(torch.cat(self.dev).cpu().numpy())       # (the one wait for the device)
        self.dev, self.waiting = [], 0

    def result(self):
        self.flush()
        return np.concatenate(self.host) if self.host else np.zeros((0,) + self.shape, np.int64)


# ------------------------------------------------------------------------------------------------------------------ scoring
def score_cams(names, cam_out_dir, gt, thresholds=None, gt_rule=0):
    """-> int64 [N, T+1, 2]: per name the ops.score_maps histogram of cam_out_dir/{name}.npy against the name's ref"""
    import torch
    from . import ops
    thr = thresholds if isinstance(thresholds, ops.ScoreThresholds) else ops.ScoreThresholds(
        default_thresholds() if thresholds is None else thresholds)
    recs = gt.of_names(names)
    out = _Gather((len(thr) + 1, 2))
    maps = _read_ahead(_read_cam, ((os.path.join(cam_out_dir, f"{n}.npy"), r[2], r[3]) for n, r in zip(names, recs)))
    for a, b in _groups(recs):
        stack = np.stack([next(maps) for _ in range(a, b)])
        out.add(ops.score_maps(torch.from_numpy(stack).to(gt.device), gt.arena, [r[:2] for r in recs[a:b]], thr, gt_rule=gt_rule))
    return out.result()


def _rows3(hist, rows):
    """[256,2] -> [3,2]: the two rows named, and everything else of `rows[2]:` summed"""
    import torch
    return torch.stack([hist[rows[0]], hist[rows[1]], hist[rows[2]:].sum(0)])


def score_labels(names, ir_label_out_dir, gt, gt_rule=0):
    """-> int64 [N, 3, 2]: per name the pixels with label 0, 1, 255 (rows) x ground-truth bit, of ir_label_out_dir/{name}.png"""
    import torch
    from . import ops
    recs = gt.of_names(names)
    out = _Gather((3, 2))
    labs = _read_ahead(_read_label, ((os.path.join(ir_label_out_dir, f"{n}.png"), r[2], r[3]) for n, r in zip(names, recs)))
    for (lo, hi, h, w, _), lab in zip(recs, labs):
        hist = ops.score_counts(torch.from_numpy(lab).to(gt.device), gt.arena, lo, hi, h, w, gt_rule=gt_rule)
        out.add(_rows3(hist, (0, 1, 255)))
    return out.result()


def score_masks(names, ins_seg_out_dir, gt, gt_rule=0):
    """-> (int64 [N, 3, 2]: per name the pixels whose mask sum is 0, 1, above 1 (rows) x ground-truth bit, of the 'mask' stack in
    ins_seg_out_dir/{name}.npy; int64 [N]: the number of masks K of each name)"""
    import torch
    from . import ops
    recs = gt.of_names(names)
    out, Ks = _Gather((3, 2)), []
    stacks = _read_ahead(_read_masks, ((os.path.join(ins_seg_out_dir, f"{n}.npy"), r[2], r[3]) for n, r in zip(names, recs)))
    for (lo, hi, h, w, _), stack in zip(recs, stacks):
        Ks.append(stack.shape[0])
        dev = torch.from_numpy(stack).to(gt.device) if stack.shape[0] else torch.empty(0, h, w, dtype=torch.uint8, device=gt.device)
        out.add(_rows3(ops.score_counts(dev, gt.arena, lo, hi, h, w, gt_rule=gt_rule), (0, 1, 2)))
    return out.result(), np.asarray(Ks, np.int64)


def score_masks_train(names, ins_seg_out_dir, gt, size, gt_rule=0):
    """score_masks on the size x size grid Stage 2 trains on: Image.NEAREST of the mask sum against Image.NEAREST of the target
    (dataset/ReferDataset.py:178-187) read the same source pixel for an output pixel, so this is rows 0 .. 2 of ops.score_planes on
    that grid of source pixels; neither resized image is formed.  -> (int64 [N, 3, 2], int64 [N])"""
    import torch
    from . import ops
    recs = gt.of_names(names)
    out, Ks = _Gather((3, 2)), []
    stacks = _read_ahead(_read_masks, ((os.path.join(ins_seg_out_dir, f"{n}.npy"), r[2], r[3]) for n, r in zip(names, recs)))
    for (lo, hi, h, w, _), stack in zip(recs, stacks):
        Ks.append(stack.shape[0])
        dev = torch.from_numpy(stack).to(gt.device) if stack.shape[0] else torch.empty(0, h, w, dtype=torch.uint8, device=gt.device)
        out.add(ops.score_planes(dev, gt.arena, lo, hi, h, w, out_hw=size, gt_rule=gt_rule)[:3])
    return out.result(), np.asarray(Ks, np.int64)


def score_instances(names, ins_seg_out_dir, gt, size=None, gt_rule=0):
    """per name a dict: 'table' int64 [K+3, 2], the ops.score_planes table of the whole 'mask' stack of ins_seg_out_dir/{name}.npy
    against the name's ref (rows: sum 0, 1, above 1, then one per instance); 'scored' int64 [3, 2], rows 0 .. 2 of the planes with
    score > 0 alone (the table's own when no score is <= 0, else a second ops.score_planes call on that sub-stack); 'K'; 'score'
    float64 [K].  size=S: the tables of the S x S grid Stage 2 trains on (the source pixels Pillow's NEAREST resize reads)."""
    import torch
    from . import ops
    recs = gt.of_names(names)
    files = _read_ahead(_read_instances, ((os.path.join(ins_seg_out_dir, f"{n}.npy"), r[2], r[3]) for n, r in zip(names, recs)))
    waiting, flat, scores = [], [], []

    def flush():
        if waiting:
            flat.append(torch.cat(waiting).cpu().numpy())           # (the one wait for the device)
            del waiting[:]
    for (lo, hi, h, w, _), (stack, score) in zip(recs, files):
        dev = torch.from_numpy(stack).to(gt.device) if stack.shape[0] else torch.empty(0, h, w, dtype=torch.uint8, device=gt.device)
        table = ops.score_planes(dev, gt.arena, lo, hi, h, w, out_hw=size, gt_rule=gt_rule)
        keep = score > 0
        if keep.all():
            scored = table[:3]
        else:                                                      # (an index list from the host: no wait for the device)
            sub = dev.index_select(0, torch.from_numpy(np.nonzero(keep)[0]).to(gt.device))
            scored = ops.score_planes(sub, gt.arena, lo, hi, h, w, out_hw=size, gt_rule=gt_rule)[:3]
        waiting += [table, scored]
        scores.append(score)
        if len(waiting) >= 2 * FLUSH:
            flush()
    flush()
    flat = np.concatenate(flat) if flat else np.zeros((0, 2), np.int64)
    out, at = [], 0
    for score in scores:
        K = score.size
        out.append({"table": flat[at:at + K + 3], "scored": flat[at + K + 3:at + K + 6], "K": K, "score": score})
        at += K + 6
    return out


# ------------------------------------------------------------------------------------------------------------------ numbers
def _ratio(num, den):
    return float(num) / float(den) if den > 0 else None


def _miou_oiou(I, U):
    """per-name I, U int64 [N] -> (100 mean(I/U, 0 where U is 0), 100 sum I / max(sum U, 1)); (None, None) without names"""
    if I.size == 0:
        return None, None
    iou = np.where(U > 0, I / np.maximum(U, 1), 0.0)
    return float(100.0 * iou.mean()), float(100.0 * I.sum() / max(int(U.sum()), 1))


def sweep_iu(hist):
    """int64 [N, T+1, 2] -> (I, U) int64 [N, T]: I[j] = sum_{b>j} h[b][1], U[j] = sum_{b>j} h[b][0] + sum_b h[b][1]"""
    hist = np.asarray(hist, np.int64)
    above = np.cumsum(hist[:, ::-1], axis=1)[:, ::-1][:, 1:]         # [N, T, 2]: bins b > j
    return above[:, :, 1], above[:, :, 0] + hist[:, :, 1].sum(1, keepdims=True)


def summarise_cams(hist, thresholds):
    """-> dict: thresholds, mIoU[t], oIoU[t], the best threshold by mIoU (the first on ties), names"""
    thresholds = [float(t) for t in thresholds]
    I, U = sweep_iu(hist)
    assert I.shape[1] == len(thresholds), (I.shape, len(thresholds))
    pairs = [_miou_oiou(I[:, j], U[:, j]) for j in range(len(thresholds))]
    miou, oiou = [p[0] for p in pairs], [p[1] for p in pairs]
    best = None if I.shape[0] == 0 else int(np.argmax(np.asarray(miou)))          # (argmax: the first of equal maxima)
    return {"names": int(I.shape[0]), "thresholds": thresholds, "mIoU": miou, "oIoU": oiou,
            "best_threshold": None if best is None else thresholds[best], "best_mIoU": None if best is None else miou[best]}


def labels_iu(hist3):
    """int64 [N,3,2] (label 0, 1, 255) -> (I, U) of label == 1"""
    h = np.asarray(hist3, np.int64)
    return h[:, 1, 1], h[:, 1, 0] + h[:, :, 1].sum(1)


def summarise_labels(hist3):
    """-> dict: mIoU / oIoU of label == 1, fg_precision n(1 & gt)/n(1), bg_precision n(0 & ~gt)/n(0), fg_recall n(1 & gt)/n(gt),
    ignored_share n(255)/n, over all names' pixels; a ratio with a zero denominator is None"""
    h = np.asarray(hist3, np.int64).reshape(-1, 3, 2)
    I, U = labels_iu(h)
    miou, oiou = _miou_oiou(I, U)
    t = h.sum(0)
    return {"names": int(h.shape[0]), "mIoU": miou, "oIoU": oiou,
            "fg_precision": _ratio(t[1, 1], t[1].sum()), "bg_precision": _ratio(t[0, 0], t[0].sum()),
            "fg_recall": _ratio(t[1, 1], t[:, 1].sum()), "ignored_share": _ratio(t[2].sum(), t.sum())}


def masks_iu(hist3):
    """int64 [N,3,2] (sum 0, 1, above 1) -> (I, U) of sum > 0"""
    h = np.asarray(hist3, np.int64)
    return h[:, 1, 1] + h[:, 2, 1], h[:, 1:, 0].sum(1) + h[:, :, 1].sum(1)


def summarise_masks(hist3, K):
    """-> dict: mIoU / oIoU of sum > 0, overlap_share n(sum > 1)/n(sum > 0), the mean K, the share of names with K = 0"""
    h = np.asarray(hist3, np.int64).reshape(-1, 3, 2)
    K = np.asarray(K, np.int64).reshape(-1)
    assert K.size == h.shape[0], (K.size, h.shape)
    I, U = masks_iu(h)
    miou, oiou = _miou_oiou(I, U)
    t = h.sum(0)
    return {"names": int(h.shape[0]), "mIoU": miou, "oIoU": oiou, "overlap_share": _ratio(t[2].sum(), t[1:].sum()),
            "mean_K": _ratio(K.sum(), K.size), "empty_share": _ratio((K == 0).sum(), K.size)}


# ------------------------------------------------------------------------------------------------------------------ instances
AP_THRESHOLDS_20 = tuple(range(10, 20))          # tau = q/20: 0.50, 0.55 ... 0.95


def instance_counts(rec):
    """one record of score_instances -> (a, i, g): a[k] the area of instance k, i[k] its intersection with the ground truth (Python
    integers), g the ground-truth area"""
    t = np.asarray(rec["table"], np.int64)
    return [int(v) for v in t[3:].sum(1)], [int(v) for v in t[3:, 1]], int(t[:3, 1].sum())


def _voc_ap(dets, n_pos, q):
    """dets in rank order: (name, a, i, g).  True positive: g > 0, 20 i >= q (a + g - i), and the first such of its name.  The area
    under the precision envelope over recall (all-point interpolation); None without a positive name."""
    if n_pos == 0:
        return None
    hit, tp, fp, curve = set(), 0, 0, []
    for name, a, i, g in dets:
        if g > 0 and 20 * i >= q * (a + g - i) and name not in hit:
            hit.add(name)
            tp += 1
        else:
            fp += 1
        curve.append((tp, tp + fp))
    ap, best = 0.0, 0.0
    for j in range(len(curve) - 1, -1, -1):                        # the envelope from the right: max precision at this recall or beyond
        best = max(best, curve[j][0] / curve[j][1])
        if curve[j][0] > (curve[j - 1][0] if j else 0):            # recall rises by 1/n_pos here
            ap += best / n_pos
    return ap


def pick_top1(score):
    """the instance of highest score, the first on ties; None without instances"""
    top = None
    for k in range(len(score)):
        if top is None or score[k] > score[top]:
            top = k
    return top


def pick_best(a, i, g):
    """the instance of highest IoU = i / (a + g - i), the first on ties; None without instances.  Python integers, compared by
    cross-multiplication: i_k u_b > i_b u_k (u = 0 only with i = 0, which then counts as an IoU of 0 on either side)"""
    best = None
    for k in range(len(a)):
        if best is None or i[k] * (a[best] + g - i[best]) > i[best] * (a[k] + g - i[k]):
            best = k
    return best


def summarise_instances(recs):
    """the records of score_instances -> dict.  A project definition (the reference names --eval_ins_seg_pass and ships no such pass):
    per instance IoU = i / (a + g - i), 0 where that is 0.  Four ways to turn a name's instances into one mask, each as mIoU / oIoU:
    top1 (the highest score, the first on ties), best (the highest IoU, compared as exact fractions, the first on ties), scored (the
    union of the planes with score > 0), union (all planes: the 'masks' numbers).  K = 0: I = 0, U = g.  zero_score_share = the
    share of instances with score <= 0, zero_score_fp_share = their share of sum (a - i); a ratio with a zero denominator is None.
    ap50 / ap75 / ap (the mean over 0.50, 0.55 ... 0.95): the VOC detection rule restated, one ground-truth object per name --
    detections by score descending (float64; ties by the name's position, then the plane), a true positive iff g > 0, IoU >= tau in
    integers and no earlier one of its name, all-point interpolation, None when no name has g > 0."""
    I = {k: [] for k in ("top1", "best", "scored", "union")}
    U = {k: [] for k in I}
    dets, n_pos, n_inst, n_zero, fp_all, fp_zero = [], 0, 0, 0, 0, 0
    for n, rec in enumerate(recs):
        a, i, g = instance_counts(rec)
        score = [float(s) for s in rec["score"]]
        assert len(a) == len(score) == rec["K"], (len(a), len(score), rec["K"])
        n_pos += g > 0
        top, best = pick_top1(score), pick_best(a, i, g)
        for k in range(len(a)):
            dets.append((-score[k], n, k, a[k], i[k], g))
            n_inst += 1
            fp_all += a[k] - i[k]
            if score[k] <= 0:
                n_zero += 1
                fp_zero += a[k] - i[k]
        for key, k in (("top1", top), ("best", best)):
            I[key].append(0 if k is None else i[k])
            U[key].append(g if k is None else a[k] + g - i[k])
        for key, h in (("scored", rec["scored"]), ("union", np.asarray(rec["table"])[:3])):
            pi, pu = masks_iu(np.asarray(h, np.int64)[None])
            I[key].append(int(pi[0]))
            U[key].append(int(pu[0]))
    out = {"names": len(recs), "instances": n_inst}
    for key in ("top1", "best", "scored", "union"):
        m, o = _miou_oiou(np.asarray(I[key], np.int64), np.asarray(U[key], np.int64))
        out[key] = {"mIoU": m, "oIoU": o}
    out["zero_score_share"] = _ratio(n_zero, n_inst)
    out["zero_score_fp_share"] = _ratio(fp_zero, fp_all)
    dets.sort(key=lambda d: d[:3])
    ranked = [(n, a, i, g) for _, n, _, a, i, g in dets]
    aps = [_voc_ap(ranked, n_pos, q) for q in AP_THRESHOLDS_20]
    out["n_pos"] = int(n_pos)
    out["ap50"], out["ap75"] = aps[0], aps[5]
    out["ap"] = None if n_pos == 0 else sum(aps) / len(aps)
    return out


def instance_arrays(recs):
    """the per-instance integers of all names, flat: inst_offsets int64 [N+1], inst_score float64, inst_area, inst_inter int64 (the
    instances of name n are offsets[n] .. offsets[n+1]-1), inst_gt_area int64 [N]"""
    off, score, area, inter, gts = [0], [], [], [], []
    for rec in recs:
        a, i, g = instance_counts(rec)
        off.append(off[-1] + len(a))
        score += [float(s) for s in rec["score"]]
        area += a
        inter += i
        gts.append(g)
    return {"inst_offsets": np.asarray(off, np.int64), "inst_score": np.asarray(score, np.float64),
            "inst_area": np.asarray(area, np.int64), "inst_inter": np.asarray(inter, np.int64), "inst_gt_area": np.asarray(gts, np.int64)}
