"""numpy + torch-CPU restatement of the reference's box metrics (validate.py:106-117, 191-208, 226-247;
utils/box_eval_utils.py:10-73; utils/box_utils.py:50-63) on the boolean mask `validate` hands to generate_bbox.

On a 0/1 input, generate_bbox is: (1) an all-zero / all-one mask gives the default list (min-max normalisation is 0/0, the
colour map sends NaN to black, nothing survives the threshold); (2) one proposal (x, y, w, h) per contour of
findContours(RETR_TREE) = the bounding rectangle of every 8-connected foreground component and, for every hole (a 4-connected
background component that does not reach the frame), the hole's rectangle grown by one pixel (OpenCV >= 3.2, which does not clear
the outer pixel ring); (3) confidence = uint8 slice mean / 255; (4) torchvision's CPU NMS on the (x, y, w, h) rows read as
(x1, y1, x2, y2); (5) survivors with confidence > 0.5 * max over all proposals, as (x, y, x + w, y + h, conf).

PROJECT RULE (not a reference fact): proposals of equal float32 confidence are visited in ascending raster index of the
component's / the hole's first pixel.  cv2's contour order and the stability of torchvision's sort cannot be observed on this
stack, so this restatement -- not a recording of cv2 / torchvision -- is what the device pass is pinned to.

No cv2, no torchvision, no scipy; flood fill for the labelling.
"""
import numpy as np
import torch

DEFAULT = [[0, 0, 1, 1, 0], [0, 0, 1, 1, 0]]


def _flood(mask, seen, y0, x0, eight):
    """pixels of the component of (y0, x0) among pixels equal to mask[y0, x0]"""
    H, W = mask.shape
    c = mask[y0, x0]
    stack = [(y0, x0)]
    seen[y0, x0] = True
    out = []
    nb = ((-1, 0), (1, 0), (0, -1), (0, 1)) + (((-1, -1), (-1, 1), (1, -1), (1, 1)) if eight else ())
    while stack:
        y, x = stack.pop()
        out.append((y, x))
        for dy, dx in nb:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and not seen[yy, xx] and mask[yy, xx] == c:
                seen[yy, xx] = True
                stack.append((yy, xx))
    return out


def proposals(mask):
    """-> [(x, y, w, h)] in raster order of each component's / hole's first pixel, [] for a degenerate mask"""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    if mask.all() or not mask.any():
        return []
    seen = np.zeros((H, W), bool)
    out = []
    for y in range(H):
        for x in range(W):
            if seen[y, x]:
                continue
            fg = bool(mask[y, x])
            px = _flood(mask, seen, y, x, eight=fg)
            ys = [p[0] for p in px]
            xs = [p[1] for p in px]
            y0, y1, x0, x1 = min(ys), max(ys), min(xs), max(xs)
            if fg:
                out.append((x0, y0, x1 - x0 + 1, y1 - y0 + 1))
            elif y0 > 0 and x0 > 0 and y1 < H - 1 and x1 < W - 1:            # a hole: does not reach the frame
                out.append((x0 - 1, y0 - 1, x1 - x0 + 3, y1 - y0 + 3))
    return out


def confidences(mask, props):
    g = (np.asarray(mask) != 0).astype(np.uint8) * 255
    return [g[y:y + h, x:x + w].mean() / 255 for (x, y, w, h) in props]


def nms(props, conf, thr=0.05):
    """torchvision's nms_kernel_impl (CPU) on float32 rows / scores; ties by ascending index (the project rule)"""
    b = np.asarray(props, np.float32).reshape(-1, 4)
    s = np.asarray(conf, np.float64).astype(np.float32)
    order = sorted(range(len(s)), key=lambda i: (-float(s[i]), i))
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    areas = (x2 - x1) * (y2 - y1)
    assert areas.dtype == np.float32
    dead = np.zeros(len(s), bool)
    rank = np.empty(len(s), np.int64)
    rank[order] = np.arange(len(s))
    keep = []
    zero = np.float32(0)
    with np.errstate(all="ignore"):
        for i in order:
            if dead[i]:
                continue
            keep.append(i)
            # (the inner loop over the later boxes, all at once: float32 one operation at a time)
            w = np.maximum(zero, np.minimum(x2[i], x2) - np.maximum(x1[i], x1))
            h = np.maximum(zero, np.minimum(y2[i], y2) - np.maximum(y1[i], y1))
            inter = w * h
            ovr = inter / ((areas[i] + areas) - inter)
            assert ovr.dtype == np.float32
            dead |= (ovr.astype(np.float64) > thr) & (rank > rank[i])
    return keep


def generate_bbox(mask, full=False):
    """-> the reference's list [(x1, y1, x2, y2, conf)]; full=True: (list, dict of the intermediate results)"""
    props = proposals(mask)
    info = {"props": props, "n_nms": 0, "kept_rows": [], "cmax": 0.0}
    if not props:
        return ([list(b) for b in DEFAULT], info) if full else [list(b) for b in DEFAULT]
    conf = confidences(mask, props)
    keep = nms(props, conf)
    cmax = float(np.max(conf))
    m = np.asarray(mask) != 0
    out = []
    for i in keep:
        if conf[i] > 0.5 * cmax:
            x, y, w, h = props[i]
            out.append((float(x), float(y), float(x + w), float(y + h), float(conf[i])))   # (rows of a float tensor's .tolist())
            info["kept_rows"].append((x, y, w, h, int(m[y:y + h, x:x + w].sum())))
    info.update(n_nms=len(keep), cmax=cmax)
    return (out, info) if full else out


def box_iou(b1, gt):
    """utils/box_utils.box_iou of one predicted box against the one int64 ground-truth box, as torch promotes it"""
    b1 = torch.tensor([list(b1[:4])])
    b2 = torch.as_tensor(np.asarray(gt).reshape(1, 4), dtype=torch.int64)
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    lt = torch.max(b1[:, None, :2], b2[:, :2])
    rb = torch.min(b1[:, None, 2:], b2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = a1[:, None] + a2 - inter
    return torch.sum(torch.diag(inter / union))


def sentence(mask, target, gt_box, argmax, gen=None):
    """steps 1-6 for one (image, sentence); argmax = (my, mx); gen: a generate_bbox(mask, full=True) result to reuse.
    -> dict with every field of the device record"""
    boxes, info = gen if gen is not None else generate_bbox(mask, full=True)
    my, mx = int(argmax[0]), int(argmax[1])
    hit = boxes[0]
    for bb in boxes:
        if bb[0] <= mx <= bb[2] and bb[1] <= my <= bb[3]:
            hit = bb
    miou = box_iou(hit, gt_box)
    acc = 0
    for bb in boxes:
        if box_iou(bb, gt_box) > 0.5:
            acc = 1
            break
    return {"hitm": int(np.asarray(target)[my, mx] != 0), "n_prop": len(info["props"]), "n_nms": info["n_nms"],
            "n_kept": len(info["kept_rows"]), "bbox_hit": tuple(int(v) for v in hit[:4]), "box_acc": acc,
            "box_miou": np.float32(float(miou)), "cmax": info["cmax"], "boxes": [tuple(b) for b in boxes],
            "kept_rows": info["kept_rows"]}


class Meters:
    """the reference's accumulation (validate.py:192-193, 207-208, 226-229, 240-245): hitm a Python int, box_miou a float32 tensor
    sum, box_acc an int64 tensor sum, both AverageMeter means"""

    def __init__(self):
        self.n = 0
        self.hitm = 0
        self.iou_sum = 0
        self.acc_sum = 0
        self.count = 0

    def update(self, rec, n=1):
        self.n += 1
        self.hitm += rec["hitm"]
        self.iou_sum = self.iou_sum + torch.tensor(float(rec["box_miou"]), dtype=torch.float32) * n
        self.acc_sum = self.acc_sum + torch.tensor(int(rec["box_acc"])) * n
        self.count += n

    def result(self):
        return {"hitm": self.hitm / self.n * 100, "box_miou": float(100 * (self.iou_sum / self.count)),
                "box_acc": float(100 * (self.acc_sum / self.count)), "n_sent": self.n}


def blob_mask(H, W, seed, q=0.7, sigma=3.0):
    """a Gaussian-smoothed normal field thresholded at its q quantile"""
    rng = np.random.RandomState(seed)
    f = rng.randn(H, W)
    r = int(3 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    f = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="reflect"), k, "valid"), 0, f)
    f = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="reflect"), k, "valid"), 1, f)
    return f > np.quantile(f, q)
