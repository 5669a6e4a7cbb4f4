"""Score the artefacts between Stage 1 and Stage 2 against the REFER ground truth of their refs (tris_amd.pseudo_eval,
csrc/labelscore.hip):

    python -m tris_amd.eval_pseudo --refer_data_root R --dataset refcocog --splitBy umd [--split train] --train_list names.json
           [--cam_out_dir D] [--ir_label_out_dir L] [--ins_seg_out_dir O] [--cam_eval_thres t1,t2,...]
           [--eval_ins_seg_pass True] [--size S] [--out summary.json] [--per_name records.npz]

  D  the response maps validate_same_sentence(save_cam=True) saved            D/{name}.npy  float32 [H,W]
  L  the labels of tris_amd.cam_to_ir_label                                   L/{name}.png  1 / 0 / 255
  O  the instance masks of tris_amd.make_ins_seg (Stage 2's --pseudo_path)    O/{name}.npy  {'mask': bool [K,h,w]}
At least one of the three is required and each one given is scored.  The argument names are the reference's (args.py,
IRNet/run_sample_refer.py, which names --cam_eval_thres and the eval passes and ships none); the three directories have no default
here because a default would be scored.  --cam_eval_thres is a comma-separated ascending list; without it the sweep is 1e-9
(validate's own threshold: at it the command reproduces the mIoU validate printed for the same maps) and 0.05 .. 0.95.

Two opt-in passes over O (both need --ins_seg_out_dir; without them the command prints and writes what it did before):
  --eval_ins_seg_pass True   (the reference's name and form) the instances one by one, with the 'score' make_ins_seg wrote per instance:
                             summary["instances"] = top-1 / best / scored / union IoU, the score-0 fragments' share of the false-positive
                             area, AP50 / AP75 / AP by the VOC detection rule (pseudo_eval.summarise_instances: a project definition)
  --size S                   (args.py's name; no default here) summary["masks_train"] = the 'masks' numbers on the S x S grid Stage 2
                             trains on, i.e. at the source pixels Image.NEAREST reads for the mask sum and for the target
"""
import argparse
import json

import numpy as np


def get_parser():
    p = argparse.ArgumentParser(description="Score response maps, CRF labels and pseudo masks against REFER on the MI355X")
    p.add_argument("--refer_data_root", default="../../data/", type=str)
    p.add_argument("--dataset", default="refcoco", type=str)
    p.add_argument("--splitBy", default="unc", type=str)
    p.add_argument("--split", default="train", type=str)
    p.add_argument("--train_list", default="voc12/train_aug.txt", type=str, help="JSON list of names")
    p.add_argument("--cam_out_dir", default=None, type=str)
    p.add_argument("--ir_label_out_dir", default=None, type=str)
    p.add_argument("--ins_seg_out_dir", default=None, type=str)
    p.add_argument("--cam_eval_thres", default=None, type=str, help="t1,t2,... ascending (default: 1e-9, then 0.05 .. 0.95)")
    p.add_argument("--eval_ins_seg_pass", default=False, type=str2bool,
                   help="True: score the instances of --ins_seg_out_dir one by one (top-1 / best / scored / union IoU, AP)")
    p.add_argument("--size", default=None, type=int,
                   help="also score the masks of --ins_seg_out_dir on the size x size grid Stage 2 trains on (no default: it would be scored)")
    p.add_argument("--out", default=None, type=str, help="write the summary as JSON")
    p.add_argument("--per_name", default=None, type=str, help="write the per-name I/U arrays as .npz")
    return p


def str2bool(v):
    """the reference's argument form (IRNet/run_sample_refer.py:102 --eval_ins_seg_pass True)"""
    if isinstance(v, bool):
        return v
    if str(v).lower() in ("yes", "true", "t", "y", "1"):
        return True
    if str(v).lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError(f"{v!r} is neither True nor False")


def parse_thresholds(text):
    """'t1,t2,...' -> ops.ScoreThresholds (finite, strictly ascending in float32, 1 .. 64 entries); None -> the default sweep"""
    from . import ops
    from .pseudo_eval import default_thresholds
    if text is None:
        return ops.ScoreThresholds(default_thresholds())
    try:
        values = [float(t) for t in str(text).split(",")]
    except ValueError:
        raise ValueError(f"--cam_eval_thres {text!r} is not a comma-separated list of numbers") from None
    return ops.ScoreThresholds(values)


def _stub_tokenizer(text):
    import torch
    return torch.zeros(1, 1, dtype=torch.int)       # (the sentences are not scored: no vocabulary is loaded for them)


def _fmt(v):
    return "   null" if v is None else f"{v:7.3f}"


def run(args, log=print):
    import torch
    from . import ops, pseudo_eval as pe
    dirs = (args.cam_out_dir, args.ir_label_out_dir, args.ins_seg_out_dir)
    if all(d is None for d in dirs):
        raise ValueError("nothing to score: give at least one of --cam_out_dir, --ir_label_out_dir, --ins_seg_out_dir")
    thr = parse_thresholds(args.cam_eval_thres)
    ins_pass, size = bool(getattr(args, "eval_ins_seg_pass", False)), getattr(args, "size", None)
    for flag, given in (("--eval_ins_seg_pass True", ins_pass), ("--size", size is not None)):
        if given and args.ins_seg_out_dir is None:
            raise ValueError(f"{flag} scores instance masks and needs --ins_seg_out_dir")
    if size is not None and not 1 <= size <= 4096:
        raise ValueError(f"--size {size} is not a training resolution (1 .. 4096)")
    if not torch.cuda.is_available():
        raise ops.NoGpuError("tris_amd.eval_pseudo runs on MI355X only (no GPU in this process)")
    from .dataset.ReferDataset import ReferDataset
    with open(args.train_list) as f:
        names = [str(n) for n in json.load(f)]
    ds = ReferDataset(refer_data_root=args.refer_data_root, dataset=args.dataset, splitBy=args.splitBy, split=args.split,
                      eval_mode=True, tokenizer=_stub_tokenizer)
    gt = pe.GroundTruth(ds, pe.resolve_names(names, ds))
    summary = {"dataset": args.dataset, "splitBy": args.splitBy, "split": args.split, "names": len(names)}
    per_name = {"names": np.asarray(names)}
    if args.cam_out_dir is not None:
        hist = pe.score_cams(names, args.cam_out_dir, gt, thr)
        s = summary["cams"] = pe.summarise_cams(hist, thr.given)
        per_name["cam_thresholds"] = thr.host
        per_name["cam_I"], per_name["cam_U"] = pe.sweep_iu(hist)
        log(f"response maps ({args.cam_out_dir}), {s['names']} names\n  threshold    mIoU    oIoU")
        for t, m, o in zip(s["thresholds"], s["mIoU"], s["oIoU"]):
            log(f"  {t:9.3g} {_fmt(m)} {_fmt(o)}" + ("   <- best mIoU" if t == s["best_threshold"] else ""))
    if args.ir_label_out_dir is not None:
        hist = pe.score_labels(names, args.ir_label_out_dir, gt)
        s = summary["labels"] = pe.summarise_labels(hist)
        per_name["label_I"], per_name["label_U"] = pe.labels_iu(hist)
        per_name["label_hist"] = hist
        log(f"CRF labels ({args.ir_label_out_dir}), {s['names']} names\n     mIoU    oIoU fg_prec bg_prec fg_rec ignored")
        log("  " + " ".join(_fmt(s[k] if k in ("mIoU", "oIoU") or s[k] is None else 100 * s[k])
                            for k in ("mIoU", "oIoU", "fg_precision", "bg_precision", "fg_recall", "ignored_share")) + "   (percent)")
    if args.ins_seg_out_dir is not None:
        hist, K = pe.score_masks(names, args.ins_seg_out_dir, gt)
        s = summary["masks"] = pe.summarise_masks(hist, K)
        per_name["mask_I"], per_name["mask_U"] = pe.masks_iu(hist)
        per_name["mask_hist"], per_name["mask_K"] = hist, K
        log(f"instance masks ({args.ins_seg_out_dir}), {s['names']} names\n     mIoU    oIoU overlap  mean K   K = 0")
        log("  " + " ".join(_fmt(v) for v in (s["mIoU"], s["oIoU"], None if s["overlap_share"] is None else 100 * s["overlap_share"],
                                              s["mean_K"], None if s["empty_share"] is None else 100 * s["empty_share"])))
        if size is not None:
            hist, K = pe.score_masks_train(names, args.ins_seg_out_dir, gt, size)
            s = summary["masks_train"] = pe.summarise_masks(hist, K)
            per_name["mask_train_hist"] = hist
            log(f"instance masks at {size} x {size}, NEAREST as Stage 2 resizes them\n     mIoU    oIoU overlap")
            log("  " + " ".join(_fmt(v) for v in (s["mIoU"], s["oIoU"], None if s["overlap_share"] is None else 100 * s["overlap_share"])))
        if ins_pass:
            recs = pe.score_instances(names, args.ins_seg_out_dir, gt)
            s = summary["instances"] = pe.summarise_instances(recs)
            if args.per_name is not None:
                per_name.update(pe.instance_arrays(recs))
            pct = lambda v: None if v is None else 100 * v
            log(f"instances one by one, {s['instances']} of {s['names']} names (a project definition)\n   policy    mIoU    oIoU")
            for key in ("top1", "best", "scored", "union"):
                log(f"  {key:>7s} {_fmt(s[key]['mIoU'])} {_fmt(s[key]['oIoU'])}")
            log("     AP50    AP75      AP  score<=0  their share of false-positive area   (percent)")
            log("  " + " ".join(_fmt(pct(s[k])) for k in ("ap50", "ap75", "ap", "zero_score_share", "zero_score_fp_share")))
    if args.out is not None:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    if args.per_name is not None:
        np.savez(args.per_name, **per_name)
    return summary


def main(argv=None):
    args = get_parser().parse_args(argv)
    try:
        run(args)
    except (FileNotFoundError, ValueError, TypeError) as e:
        raise SystemExit(f"eval_pseudo: {e}")


if __name__ == "__main__":
    main()
