"""numpy restatement of csrc/labelscore.hip and of tris_amd.pseudo_eval's aggregation, for tests/test_pseudo_eval_host.py and
tests/test_gpu_pseudo_eval.py.  Ground-truth counts come from rle_arena.decode_sum_numpy (or from a mask the caller rasterised on
the host), histograms from plain boolean counting, thresholds are compared in float32.  Written with loops over names and
thresholds on purpose: nothing here shares code with the module under test."""
import numpy as np

from tris_amd.dataset.rle_arena import decode_sum_numpy


def gt_bits(ends, seg_off, ranges, H, W, gt_rule):
    """bool [K,H,W]: gt_rule 0 -> covered by exactly one segment, 1 -> covered at all"""
    c = decode_sum_numpy(np.asarray(ends), np.asarray(seg_off), [tuple(int(v) for v in r) for r in ranges], H, W)
    return (c == 1) if gt_rule == 0 else (c != 0)


def maps_hist(maps, bits, thresholds):
    """maps float32 [G,H,W], bits bool [G,H,W] -> int64 [G,T+1,2]: bin = the number of thresholds t with value > t (float32)"""
    maps = np.asarray(maps, np.float32)
    thr = np.asarray(thresholds, np.float32)
    out = np.zeros((maps.shape[0], thr.size + 1, 2), np.int64)
    for g in range(maps.shape[0]):
        with np.errstate(invalid="ignore"):
            b = np.zeros(maps[g].shape, np.int64)
            for t in thr:
                b += maps[g] > t
        for k in range(thr.size + 1):
            out[g, k, 1] = np.count_nonzero((b == k) & bits[g])
            out[g, k, 0] = np.count_nonzero((b == k) & ~bits[g])
    return out


def counts_hist(stack, bits):
    """stack uint8 [K,H,W], bits bool [H,W] -> int64 [256,2] by the byte sum over K"""
    stack = np.asarray(stack, np.uint8)
    s = stack.sum(0, dtype=np.uint8) if stack.shape[0] else np.zeros(bits.shape, np.uint8)
    out = np.zeros((256, 2), np.int64)
    for v in range(256):
        out[v, 1] = np.count_nonzero((s == v) & bits)
        out[v, 0] = np.count_nonzero((s == v) & ~bits)
    return out


def iu(pred, gt):
    return int(np.count_nonzero(pred & gt)), int(np.count_nonzero(pred | gt))


def means(IU):
    """[(I, U)] -> (mIoU, oIoU) by tris_amd.validate's rule: iou = I/U if U > 0 else 0"""
    if not IU:
        return None, None
    ious = [(i / u if u > 0 else 0.0) for i, u in IU]
    return 100.0 * sum(ious) / len(ious), 100.0 * sum(i for i, _ in IU) / max(sum(u for _, u in IU), 1)


def ratio(a, b):
    return a / b if b > 0 else None


def cams_summary(maps, gts, thresholds):
    """maps: list of float32 [H,W]; gts: list of bool [H,W]"""
    thr = np.asarray(thresholds, np.float32)
    miou, oiou = [], []
    for t in thr:
        with np.errstate(invalid="ignore"):
            m, o = means([iu(np.asarray(c, np.float32) > t, g) for c, g in zip(maps, gts)])
        miou.append(m)
        oiou.append(o)
    best = None
    for j, m in enumerate(miou):
        if m is not None and (best is None or m > miou[best]):
            best = j
    return {"names": len(maps), "thresholds": [float(t) for t in thresholds], "mIoU": miou, "oIoU": oiou,
            "best_threshold": None if best is None else float(thresholds[best]), "best_mIoU": None if best is None else miou[best]}


def labels_summary(labels, gts):
    m, o = means([iu(l == 1, g) for l, g in zip(labels, gts)])
    n1 = sum(int((l == 1).sum()) for l in labels)
    n0 = sum(int((l == 0).sum()) for l in labels)
    n255 = sum(int((l == 255).sum()) for l in labels)
    hit = sum(int(((l == 1) & g).sum()) for l, g in zip(labels, gts))
    bg = sum(int(((l == 0) & ~g).sum()) for l, g in zip(labels, gts))
    return {"names": len(labels), "mIoU": m, "oIoU": o, "fg_precision": ratio(hit, n1), "bg_precision": ratio(bg, n0),
            "fg_recall": ratio(hit, sum(int(g.sum()) for g in gts)), "ignored_share": ratio(n255, sum(l.size for l in labels))}


def masks_summary(stacks, gts):
    sums = [s.astype(np.int64).sum(0) if s.shape[0] else np.zeros(g.shape, np.int64) for s, g in zip(stacks, gts)]
    m, o = means([iu(s > 0, g) for s, g in zip(sums, gts)])
    K = [s.shape[0] for s in stacks]
    return {"names": len(stacks), "mIoU": m, "oIoU": o,
            "overlap_share": ratio(sum(int((s > 1).sum()) for s in sums), sum(int((s > 0).sum()) for s in sums)),
            "mean_K": ratio(sum(K), len(K)), "empty_share": ratio(sum(k == 0 for k in K), len(K))}


def hist_of_labels(labels, gts):
    """-> int64 [N,3,2], rows label 0, 1, 255"""
    return np.array([[[np.count_nonzero((l == v) & (g == bit)) for bit in (False, True)] for v in (0, 1, 255)]
                     for l, g in zip(labels, gts)], np.int64).reshape(-1, 3, 2)


def hist_of_masks(stacks, gts):
    """-> int64 [N,3,2], rows sum 0, 1, above 1"""
    out = []
    for s, g in zip(stacks, gts):
        t = s.astype(np.int64).sum(0) if s.shape[0] else np.zeros(g.shape, np.int64)
        out.append([[np.count_nonzero(sel & (g == bit)) for bit in (False, True)] for sel in (t == 0, t == 1, t > 1)])
    return np.array(out, np.int64).reshape(-1, 3, 2)
