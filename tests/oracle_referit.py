"""Fixture and restatement for the ReferIt evaluation (tris_amd.validate_referit, tris_amd.dataset.Dataset_referit,
csrc/referit.hip).

`synthetic_root(dir)` writes a tiny ReferIt tree -- annotations/{test,train}.pickle and images/*.jpg.  The images are seeded-RNG
arrays saved LOSSLESSLY: PNG bytes under the .jpg name (Pillow identifies a format by content), so decoding gives the same bytes
on every machine.  What the tree holds (tests/golden/g19_referit.npz is the reference's ImageLoader / ImageLoader_train on it):

  1001  37 x 50   0 `on`: one segment around the aim point, a box around it            1 fails the 5 % rule (a gap in the keys)
                  2 `double`: two overlapping segments over the aim point (counts 2)   3 `off`: target and box in the far corner
  1002  64 x 48   a grey image (mode L)   0 a segment whose first count is 0   1 a segment with an interior zero run
                  2 a compressed-string RLE
  1003  33 x 47   every annotation fails the 5 % rule
  1004  80 x 100  0 `second`: two boxes, only the second holds the aim point   1 a box of EXACTLY 0.05*H*W (dropped: the rule is >)
                  2 `on`

`aims` ({(key, annotation index): (y, x)}) moves the aimed annotations: the end-to-end test takes the arg-max points from a first
pass so that both values of Hit and HitM occur; without it the aim is the image centre.

`restate(items, cams)` is validate_referit.py:143-226 in numpy over dumped cams.
"""
import io
import os
import pickle

import numpy as np

SIZES = {"1001": (37, 50), "1002": (64, 48), "1003": (33, 47), "1004": (80, 100)}
GREY = "1002"
AIMED = [("1001", 0), ("1001", 2), ("1001", 3), ("1004", 0), ("1004", 2)]


# ------------------------------------------------------------------------------------------------------------------ RLE forms
def counts_of(mask):
    """column-major run lengths of a boolean mask, background first (the first count is 0 where the mask starts in foreground)"""
    v = np.asarray(mask, bool).reshape(-1, order="F")
    edges = np.nonzero(v[1:] != v[:-1])[0] + 1
    runs = np.diff(np.concatenate([[0], edges, [v.size]])).tolist()
    return ([0] + runs) if v[0] else runs


def with_zero_run(counts, at=1):
    """the same mask with run `at` split in two by a zero-length run of the other value"""
    c = list(counts)
    a = c[at] // 2
    return c[:at] + [a, 0, c[at] - a] + c[at + 1:]


def counts_to_string(counts):
    """maskApi.c rleToString: 5 bits per character, continuation bit 0x20, counts from the fourth on as differences"""
    out = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rect_mask(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def rle(mask, form="plain"):
    H, W = mask.shape
    c = counts_of(mask)
    if form == "zero_run":
        c = with_zero_run(c)
    if form == "string":
        c = counts_to_string(c)
    return {"size": [H, W], "counts": c}


# ------------------------------------------------------------------------------------------------------------------ the tree
def _near(H, W, y, x):
    return max(y - H // 4, 0), min(y + H // 4, H - 1), max(x - W // 4, 0), min(x + W // 4, W - 1)


def _far(H, W, y, x):
    cy, cx = (0 if y >= H // 2 else H - 1), (0 if x >= W // 2 else W - 1)
    y0, y1 = (0, H // 3) if cy == 0 else (H - 1 - H // 3, H - 1)
    x0, x1 = (0, W // 3) if cx == 0 else (W - 1 - W // 3, W - 1)
    return y0, y1, x0, x1


def _box(r):
    y0, y1, x0, x1 = r
    return [x0, y0, x1, y1]


def annotations(aims=None):
    aims = aims or {}

    def aim(key, i):
        H, W = SIZES[key]
        return aims.get((key, i), (H // 2, W // 2))

    def ann(key, query, boxes, masks, forms=None):
        forms = forms or ["plain"] * len(masks)
        return {"image_id": key, "query": query, "bbox": boxes, "segmentation": [rle(m, f) for m, f in zip(masks, forms)]}

    out = {}
    # 1001
    key = "1001"
    H, W = SIZES[key]
    n0, n2 = _near(H, W, *aim(key, 0)), _near(H, W, *aim(key, 2))
    y, x = aim(key, 2)
    inner = (max(y - 3, 0), min(y + 3, H - 1), max(x - 3, 0), min(x + 3, W - 1))
    f3 = _far(H, W, *aim(key, 3))
    out[key] = {"annotations": [
        ann(key, "the tree on the left", [_box(n0)], [rect_mask(H, W, *n0)]),
        ann(key, "a small stone", [[2, 2, 8, 9]], [rect_mask(H, W, 2, 9, 2, 8)]),
        ann(key, "two people standing close together", [_box(n2)], [rect_mask(H, W, *n2), rect_mask(H, W, *inner)]),
        ann(key, "sky", [_box(f3)], [rect_mask(H, W, *f3)]),
    ]}
    # 1002 (grey): fixed annotations, one per RLE form
    key = "1002"
    H, W = SIZES[key]
    out[key] = {"annotations": [
        ann(key, "the wall in the top left corner", [[0, 0, 20, 30]], [rect_mask(H, W, 0, 30, 0, 20)]),
        ann(key, "window", [[10, 12, 40, 50]], [rect_mask(H, W, 12, 50, 10, 40)], ["zero_run"]),
        ann(key, "the dark door on the right side of the house", [[25, 5, 47, 60]], [rect_mask(H, W, 5, 60, 25, 47)], ["string"]),
    ]}
    assert out[key]["annotations"][0]["segmentation"][0]["counts"][0] == 0
    assert 0 in out[key]["annotations"][1]["segmentation"][0]["counts"][1:]
    # 1003: nothing survives
    key = "1003"
    H, W = SIZES[key]
    out[key] = {"annotations": [
        ann(key, "bird", [[1, 1, 6, 7]], [rect_mask(H, W, 1, 7, 1, 6)]),
        ann(key, "a tiny boat", [[30, 20, 38, 28]], [rect_mask(H, W, 20, 28, 30, 38)]),
    ]}
    # 1004
    key = "1004"
    H, W = SIZES[key]
    a0 = aim(key, 0)
    far0, near0 = _far(H, W, *a0), _near(H, W, *a0)
    n2 = _near(H, W, *aim(key, 2))
    assert 0.05 * H * W == 400.0
    out[key] = {"annotations": [
        ann(key, "the road", [_box(far0), _box(near0)], [rect_mask(H, W, *far0)]),
        ann(key, "a sign exactly at the limit", [[10, 10, 30, 30]], [rect_mask(H, W, 10, 30, 10, 30)]),
        ann(key, "mountain behind the lake", [_box(n2)], [rect_mask(H, W, *n2)]),
    ]}
    return out


def image_array(key):
    H, W = SIZES[key]
    rng = np.random.RandomState(int(key))
    # (smooth + noise: a resize of pure noise would be as good, this one also has structure)
    yy, xx = np.mgrid[0:H, 0:W]
    shape = (H, W) if key == GREY else (H, W, 3)
    base = (yy * 3 + xx * 2)[..., None] if key != GREY else (yy * 3 + xx * 2)
    return ((base + rng.randint(0, 120, size=shape)) % 256).astype(np.uint8)


def synthetic_root(root, aims=None):
    """-> root; writes annotations/test.pickle, annotations/train.pickle and images/{key}.jpg (PNG bytes)"""
    from PIL import Image
    root = str(root)
    os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    ann = annotations(aims)
    with open(os.path.join(root, "annotations", "test.pickle"), "wb") as f:
        pickle.dump(ann, f, protocol=2)
    with open(os.path.join(root, "annotations", "train.pickle"), "wb") as f:
        pickle.dump({k: ann[k] for k in ("1001", "1002")}, f, protocol=2)
    for key in SIZES:
        buf = io.BytesIO()
        Image.fromarray(image_array(key)).save(buf, format="PNG")
        with open(os.path.join(root, "images", key + ".jpg"), "wb") as f:
            f.write(buf.getvalue())
    return root


# ------------------------------------------------------------------------------------------------------------------ the loop
def is_correct_hit(bbox_annot, heatmap, gt_mask):
    """validate_referit.py:104-118"""
    max_loc = np.unravel_index(np.argmax(heatmap, axis=None), heatmap.shape)
    hitm = 0
    new_gt_mask = gt_mask[max_loc[0], max_loc[1]].astype(np.int64) + 1
    if new_gt_mask.max() == 2:
        hitm = 1
    for bbox in bbox_annot:
        if bbox[0] <= max_loc[1] <= bbox[2] and bbox[1] <= max_loc[0] <= bbox[3]:
            return 1, max_loc, hitm
    return 0, max_loc, hitm


def restate(items, cams):
    """items: per image the list of its surviving sentences {"bbox": [n,4], "mask": uint8 counts [H,W]} (an empty list for an image
    without any); cams: per image the list of float32 cams [H,W] (the reference's t_cam).  -> dict of the closing line's numbers and
    the per-sentence (hit, hitm) pairs.  U == 0 gives IoU 0.0 (the project's rule; the reference divides)."""
    cum_I = cum_U = n = hit_acc = hitm_acc = 0
    iou_sum, pairs = 0, []
    for sents, cs in zip(items, cams):
        for s, cam in zip(sents, cs):
            pred = cam > np.float32(1e-9)
            target = np.asarray(s["mask"])
            I, U = int(np.logical_and(target, pred).sum()), int(np.logical_or(target, pred).sum())
            hit, _, hitm = is_correct_hit(np.asarray(s["bbox"]), cam.astype(np.float64), target)
            hit_acc += hit
            hitm_acc += hitm
            pairs.append((hit, hitm))
            cum_I += I
            cum_U += U
            iou_sum += (I / U if U > 0 else 0.0) * 1
            n += 1
    return {"oiou": 100 * float(cum_I) / max(float(cum_U), 1.0), "miou": 100 * (iou_sum / n if n else 0), "hit": 100 * hit_acc / max(n, 1),
            "hitm": hitm_acc / max(n, 1) * 100, "n_sent": n, "pairs": pairs}
