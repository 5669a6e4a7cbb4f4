"""numpy restatement of ops.score_planes (csrc/labelscore.hip) and of tris_amd.pseudo_eval's instance numbers, for
tests/test_instances_host.py and tests/test_gpu_instances.py.  Ground-truth bits come from oracle_pseudo_eval.gt_bits
(rle_arena.decode_sum_numpy) or from a mask the caller rasterised, the table from boolean counting over the sampled index grid,
the policies and the AP rule from plain Python integers, fractions and loops.  Nothing here shares code with the module under test."""
from fractions import Fraction

import numpy as np


def sample(img, yidx, xidx):
    """img [..., H, W] at the samples (yidx[y], xidx[x]); an index < 0 reads 0.  None, None: the image itself"""
    img = np.asarray(img)
    if yidx is None and xidx is None:
        return img
    yi, xi = np.asarray(yidx, np.int64), np.asarray(xidx, np.int64)
    out = img[..., np.maximum(yi, 0)[:, None], np.maximum(xi, 0)[None, :]].copy()
    out[..., yi < 0, :] = 0
    out[..., :, xi < 0] = 0
    return out


def planes_table(stack, bits, yidx=None, xidx=None):
    """stack uint8 [K,H,W], bits bool [H,W] -> int64 [K+3,2]: rows sum 0, sum 1, sum >= 2 (the sum as an integer), then one row per
    plane that is not 0; second index the ground-truth bit"""
    stack = sample(np.asarray(stack, np.uint8), yidx, xidx)
    b = sample(np.asarray(bits, bool), yidx, xidx)
    K = stack.shape[0]
    s = stack.astype(np.int64).sum(0) if K else np.zeros(b.shape, np.int64)
    sels = [s == 0, s == 1, s >= 2] + [stack[k] != 0 for k in range(K)]
    out = np.zeros((K + 3, 2), np.int64)
    for r, sel in enumerate(sels):
        out[r, 1] = np.count_nonzero(sel & b)
        out[r, 0] = np.count_nonzero(sel & ~b)
    return out


def record(stack, score, gt, yidx=None, xidx=None):
    """what pseudo_eval.score_instances returns for one name, from a bool stack [K,h,w], its scores and a rasterised ground truth"""
    stack = np.asarray(stack).astype(np.uint8)
    score = np.asarray(score, np.float64).reshape(-1)
    return {"table": planes_table(stack, gt, yidx, xidx), "scored": planes_table(stack[score > 0], gt, yidx, xidx)[:3],
            "K": stack.shape[0], "score": score}


def means(IU):
    """[(I, U)] -> (mIoU, oIoU): iou = I/U if U > 0 else 0"""
    if not IU:
        return None, None
    ious = [(i / u if u > 0 else 0.0) for i, u in IU]
    return 100.0 * sum(ious) / len(ious), 100.0 * sum(i for i, _ in IU) / max(sum(u for _, u in IU), 1)


def ratio(a, b):
    return a / b if b > 0 else None


def counts(rec):
    t = rec["table"]
    K = rec["K"]
    a = [int(t[3 + k][0]) + int(t[3 + k][1]) for k in range(K)]
    i = [int(t[3 + k][1]) for k in range(K)]
    g = int(t[0][1]) + int(t[1][1]) + int(t[2][1])
    return a, i, g


def iou(a, i, g):
    u = a + g - i
    return Fraction(i, u) if u > 0 else Fraction(0)


def ap_at(dets, n_pos, q):
    """dets in rank order [(name, a, i, g)], tau = q/20 -> AP by the VOC rule with all-point interpolation, as a Fraction"""
    if n_pos == 0:
        return None
    seen, tp, fp, prec, rec = set(), 0, 0, [], []
    for name, a, i, g in dets:
        if g > 0 and iou(a, i, g) >= Fraction(q, 20) and name not in seen:
            seen.add(name)
            tp += 1
        else:
            fp += 1
        prec.append(Fraction(tp, tp + fp))
        rec.append(Fraction(tp, n_pos))
    mrec, mpre = [Fraction(0)] + rec + [Fraction(1)], [Fraction(0)] + prec + [Fraction(0)]
    for j in range(len(mpre) - 2, -1, -1):
        mpre[j] = max(mpre[j], mpre[j + 1])
    return sum((mrec[j + 1] - mrec[j]) * mpre[j + 1] for j in range(len(mrec) - 1))


def ranked(recs):
    dets = []
    for n, rec in enumerate(recs):
        a, i, g = counts(rec)
        for k in range(rec["K"]):
            dets.append((float(rec["score"][k]), n, k, a[k], i[k], g))
    order = sorted(range(len(dets)), key=lambda j: (-dets[j][0], dets[j][1], dets[j][2]))
    return [(dets[j][1], dets[j][3], dets[j][4], dets[j][5]) for j in order]


def ap_fractions(recs):
    """-> {q: AP at tau = q/20 as a Fraction or None}, q = 10 .. 19"""
    n_pos = sum(1 for rec in recs if counts(rec)[2] > 0)
    dets = ranked(recs)
    return {q: ap_at(dets, n_pos, q) for q in range(10, 20)}


def instances_summary(recs):
    pol = {"top1": [], "best": [], "scored": [], "union": []}
    n_inst = n_zero = fp_all = fp_zero = 0
    for rec in recs:
        a, i, g = counts(rec)
        K, score = rec["K"], [float(s) for s in rec["score"]]
        if K == 0:
            pol["top1"].append((0, g))
            pol["best"].append((0, g))
        else:
            top = max(range(K), key=lambda k: (score[k], -k))
            best = max(range(K), key=lambda k: (iou(a[k], i[k], g), -k))
            pol["top1"].append((i[top], a[top] + g - i[top]))
            pol["best"].append((i[best], a[best] + g - i[best]))
        for key, h in (("scored", rec["scored"]), ("union", rec["table"])):
            pred_gt, pred_bg = int(h[1][1]) + int(h[2][1]), int(h[1][0]) + int(h[2][0])
            pol[key].append((pred_gt, pred_bg + int(h[0][1]) + pred_gt))            # U = predicted background + all ground truth
        for k in range(K):
            n_inst += 1
            fp_all += a[k] - i[k]
            if score[k] <= 0:
                n_zero += 1
                fp_zero += a[k] - i[k]
    out = {"names": len(recs), "instances": n_inst}
    for key, IU in pol.items():
        m, o = means(IU)
        out[key] = {"mIoU": m, "oIoU": o}
    out["zero_score_share"], out["zero_score_fp_share"] = ratio(n_zero, n_inst), ratio(fp_zero, fp_all)
    aps = ap_fractions(recs)
    out["n_pos"] = sum(1 for rec in recs if counts(rec)[2] > 0)
    out["ap50"] = None if aps[10] is None else float(aps[10])
    out["ap75"] = None if aps[15] is None else float(aps[15])
    out["ap"] = None if aps[10] is None else float(sum(aps.values()) / 10)
    return out
