"""ReferIt (saiapr_tc-12) evaluation on MI355X -- `isCorrectHit`, `validate`, `main` with the reference's names
(validate_referit.py:41-226).  `python -m tris_amd.validate_referit` takes tris_amd.args.get_parser() unchanged:

    python -m tris_amd.validate_referit --size 320 --dataset referit --test_split test --backbone clip-RN50 \
        --max_query_len 20 --refer_data_root <root> --output <dir> --resume --pretrain <ckpt> --eval

Per image: ONE encode_visual, ONE forward_pairs over the sentences that survive the dataset's 5 % rule (under
ops.batch_invariant(): every map equals the reference's per-sentence call bit for bit), ONE decode of their run-length targets
(ops.rle_decode_sum_arena; a plain DataLoader's dense masks are uploaded instead), ONE grouped scoring (ops.eval_post_group)
and ONE host sync.

What is kept from the reference, with its lines:
  * prediction (:160-169): bilinear, align_corners=True, to (o_H, o_W); / (max + 1e-5); > 1e-9.  I and U are taken with
    logical_and / logical_or, so a target COUNT counts as != 0;
  * Hit (:115-117): any of the annotation's boxes contains the arg-max, bounds inclusive;
  * HitM (:111-113): gt_mask[max_loc] + 1 == 2 -- a count of exactly 1 scores, a pixel covered by two segments does not.  It is
    read from the fourth record word of ops.eval_post_group, not from the boxes record (csrc/boxes.hip tests != 0, validate.py's
    rule on a 0/1 target).  The difference between the two scripts is the reference's;
  * meters (:186-195): cum_I, cum_U; mIOU_meter.update(IoU, 1) per sentence; Hit and HitM divided by the number of sentences;
  * box metrics: against the FIRST ground-truth box (:153, :180-181), accumulated as tris_amd.validate does -- a float32 sum for
    box_mIOU, an integer sum for box_Acc;
  * an image with no surviving sentence is counted in num_steps and contributes nothing;
  * the progress line and the closing line carry the reference's fields.

Project rules:
  * U == 0 gives IoU 0.0, as tris_amd.validate does (the reference would produce NaN);
  * the return value is (overall_IoU, mIOU, hit) with the types tris_amd.validate.validate returns (float, 0-d tensor, float);
  * HitM is always computed; box_mIOU / box_Acc only with TRIS_EVAL_BOXES=1 (cfg.eval_boxes), through ops.eval_boxes per sentence
    on the decoded target, their records riding the same host sync.  All are read through last_metrics();
  * --distributed raises NotImplementedError: the reference's script never reduces its meters, so its multi-rank numbers are per
    rank;
  * Stage-2 models (`signed_maps`) are scored with signed=True;
  * `visualize` is accepted and unused, as in the reference.
"""
import datetime
import os
import time

import numpy as np
import torch

from . import ops
from .config import cfg
from .dataset.hbm_referit import DeviceGroup
from .utils.util import AverageMeter

_LAST = None


def last_metrics():
    """{"hitm", "box_miou", "box_acc", "n_sent"} of the last validate() call, in percent as the reference prints them; box_miou and
    box_acc are None unless cfg.eval_boxes was on"""
    return None if _LAST is None else dict(_LAST)


def isCorrectHit(bbox_annot, heatmap, gt_mask=None):
    """validate_referit.py:104-118 -> (hit, max_loc, hitm): hitm is 1 where the target COUNT at the arg-max is exactly 1"""
    max_loc = np.unravel_index(np.argmax(heatmap, axis=None), heatmap.shape)
    hitm = 0
    if gt_mask is not None and int(np.asarray(gt_mask[max_loc[0], max_loc[1]]).max()) + 1 == 2:
        hitm = 1
    for bbox in bbox_annot:
        if bbox[0] <= max_loc[1] <= bbox[2] and bbox[1] <= max_loc[0] <= bbox[3]:
            return 1, max_loc, hitm
    return 0, max_loc, hitm


def _group_of(samples, H, W, dev):
    """-> (word_ids int64 [K,L], targets uint8 [K,H,W], bboxes) on the device for either loader"""
    if isinstance(samples, DeviceGroup):
        return samples.word_ids, ops.rle_decode_sum_arena(samples.ends, samples.seg_off, samples.ranges, H, W), samples.bboxes
    items = [samples[k] for k in samples.keys()]                               # DataLoader(ImageLoader, batch_size=1)
    ids = torch.cat([torch.as_tensor(it["word_id"]).reshape(1, -1) for it in items], 0).to(torch.int64).to(dev, non_blocking=True)
    tgt = torch.stack([torch.as_tensor(it["mask"]).reshape(H, W) for it in items], 0).to(torch.uint8).to(dev, non_blocking=True)
    boxes = [np.asarray(torch.as_tensor(it["bbox"]).cpu()).reshape(-1, 4) for it in items]
    return ids, tgt, boxes


@torch.no_grad()
def validate(args, data_loader, model, local_rank=0, visualize=False):
    global _LAST
    _LAST = None
    boxes_on = bool(cfg.eval_boxes)
    num_steps = len(data_loader)
    model.eval()
    net = model.module if hasattr(model, "module") else model
    signed = bool(getattr(net, "signed_maps", False))
    dev = torch.device("cuda", local_rank)
    batch_time, mIOU_meter = AverageMeter(), AverageMeter()
    cum_I = cum_U = n_sent = hit_acc = hitmask_acc = 0
    bx = {"iou": np.float32(0), "acc": 0, "count": 0}
    end = time.time()

    def report(idx):
        more = ""
        if boxes_on:
            c = max(bx["count"], 1)
            more = f"box_mIOU {100 * float(bx['iou']) / c:.3f} | box_Acc {100 * bx['acc'] / c:.3f} | "
        etas = batch_time.avg * (num_steps - idx)
        print(f"Test: [{idx:5d}/{num_steps}] | mIOU {100 * mIOU_meter.avg:.3f} | "
              f"Overall IOU {100 * float(cum_I) / max(float(cum_U), 1.0):.3f} | Hit {hit_acc / max(n_sent, 1) * 100:.3f} | "
              f"HitM {hitmask_acc / max(n_sent, 1) * 100:.3f} | {more}eta: {datetime.timedelta(seconds=int(etas))} | "
              f"Time {batch_time.val:.3f} ({batch_time.avg:.3f})", flush=True)

    with ops.batch_invariant():
        for idx, (img, samples, image_sizes, img_path) in enumerate(data_loader):
            K = len(samples)
            if K:
                H, W = int(image_sizes[0]), int(image_sizes[1])
                img = img.to(dev, non_blocking=True)
                ids, targets, bboxes = _group_of(samples, H, W, dev)
                vis = net.encode_visual(img)                                                # once per image
                maps = net.forward_pairs(vis, ids, [0] * K, img.shape[2])                   # [K,1,S,S]
                records, cams = ops.eval_post_group(maps, targets, signed=signed, cams=boxes_on)
                if boxes_on:
                    gts = ops.eval_boxes_gt(np.stack([b[0] for b in bboxes]), device=dev)   # the first box (:153)
                    recs = [ops.eval_boxes(cams[k], targets[k], gts[k], records[k, :3]) for k in range(K)]
                    records = torch.cat([records, torch.stack(recs).view(torch.int64)], 1)  # the records ride the same sync
                vals = records.tolist()                                                     # the one host sync of the image
                for k in range(K):
                    I, U, am, cnt = vals[k][:4]
                    n_sent += 1
                    y, x = divmod(am, W)
                    for b in bboxes[k]:
                        if b[0] <= x <= b[2] and b[1] <= y <= b[3]:
                            hit_acc += 1
                            break
                    hitmask_acc += 1 if cnt + 1 == 2 else 0
                    cum_I += I
                    cum_U += U
                    mIOU_meter.update(I / U if U > 0 else 0.0, 1)
                    if boxes_on:
                        r = ops.decode_boxes_record(vals[k][4:])
                        bx["iou"] = np.float32(bx["iou"] + r["box_miou"] * np.float32(1))
                        bx["acc"] += r["box_acc"]
                        bx["count"] += 1
                    batch_time.update(time.time() - end)
                    end = time.time()
                if idx % args.print_freq == 0:
                    report(idx)
    overall_IoU = 100 * float(cum_I) / max(float(cum_U), 1.0)
    mIOU = torch.tensor(100 * float(mIOU_meter.avg))
    hit = 100 * hit_acc / max(n_sent, 1)
    _LAST = {"hitm": hitmask_acc / max(n_sent, 1) * 100, "box_miou": None, "box_acc": None, "n_sent": int(n_sent)}
    more = ""
    if boxes_on:
        cnt32 = np.float32(max(bx["count"], 1))
        _LAST["box_miou"] = float(np.float32(100) * (np.float32(bx["iou"]) / cnt32))
        _LAST["box_acc"] = float(np.float32(100) * (np.float32(bx["acc"]) / cnt32))
        more = f"  box_mIOU {_LAST['box_miou']}  box_acc {_LAST['box_acc']}"
    print(f"Test: mIOU {float(mIOU):.5f}  Overall IOU {overall_IoU:.5f}  HiT {hit:.3f}  hitmax_acc {_LAST['hitm']:.3f}{more}")
    return overall_IoU, mIOU, hit


def build_loader(args, dataset):
    """the HBM-resident evaluation set unless TRIS_HBM_LOADER=0 (then the reference's DataLoader, batch_size=1)"""
    if cfg.hbm_loader:
        from .dataset.hbm_referit import HbmReferitCache, HbmReferitLoader
        return HbmReferitLoader(HbmReferitCache(dataset, args.size))
    from torch.utils.data import DataLoader
    return DataLoader(dataset, batch_size=1, num_workers=2, pin_memory=True, shuffle=False)


def _model_class(args):
    """the reference switches stages by editing an import (validate_referit.py:8-9); here the checkpoint decides: one that holds
    the Stage-2 decoder (`reduced_c1.*`) builds model_stage2.TRIS, anything else model_stage1.TRIS"""
    path = os.path.join(args.output, args.pretrain) if (args.resume and args.pretrain is not None) else None
    if path is not None and os.path.isfile(path):
        keys = torch.load(path, map_location="cpu").get("model", {})
        if any(k.startswith("reduced_c1.") for k in keys):
            from .model.model_stage2 import TRIS
            return TRIS
    from .model.model_stage1 import TRIS
    return TRIS


def main(args):
    if args.distributed:
        raise NotImplementedError("validate_referit: --distributed is not provided (the reference's script never reduces its meters "
                                  "across ranks, so its multi-rank numbers are per rank); run one process")
    from .dataset.Dataset_referit import get_refit_dataset
    from .utils.util import load_checkpoint
    model = _model_class(args)(args).cuda()
    print(f"number of params: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")
    _, val_dataset = get_refit_dataset(args)
    val_loaders = [build_loader(args, val_dataset) for _ in args.test_split.split(",")]
    if args.resume:
        if args.pretrain is not None:
            load_checkpoint(args, model)
        if args.eval:
            st = time.time()
            val_acc = testA_acc = testB_acc = 0
            for i, val_loader in enumerate(val_loaders):
                oIoU, mIoU, hit = validate(args, val_loader, model, 0)
                if i == 0:
                    val_acc = mIoU
                elif i == 1:
                    testA_acc = mIoU
                else:
                    testB_acc = mIoU
            print(f"val: {val_acc}, testA, {testA_acc}, testB: {testB_acc}")
            print(f"Testing time:  {datetime.timedelta(seconds=int(time.time() - st))}")


if __name__ == "__main__":
    from .args import get_parser
    from .train_stage1 import setup_seed
    setup_seed(1234)                      # validate_referit.py:37
    _args = get_parser().parse_args()
    print("=========" * 10)
    print(_args)
    print("=========" * 10)
    main(_args)
