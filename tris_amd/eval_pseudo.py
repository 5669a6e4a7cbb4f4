"""Score the artefacts between Stage 1 and Stage 2 against the REFER ground truth of their refs (tris_amd.pseudo_eval,
csrc/labelscore.hip):

    python -m tris_amd.eval_pseudo --refer_data_root R --dataset refcocog --splitBy umd [--split train] --train_list names.json
           [--cam_out_dir D] [--ir_label_out_dir L] [--ins_seg_out_dir O] [--cam_eval_thres t1,t2,...]
           [--out summary.json] [--per_name records.npz]

  D  the response maps validate_same_sentence(save_cam=True) saved            D/{name}.npy  float32 [H,W]
  L  the labels of tris_amd.cam_to_ir_label                                   L/{name}.png  1 / 0 / 255
  O  the instance masks of tris_amd.make_ins_seg (Stage 2's --pseudo_path)    O/{name}.npy  {'mask': bool [K,h,w]}
At least one of the three is required and each one given is scored.  The argument names are the reference's (args.py,
IRNet/run_sample_refer.py, which names --cam_eval_thres and the eval passes and ships none); the three directories have no default
here because a default would be scored.  --cam_eval_thres is a comma-separated ascending list; without it the sweep is 1e-9
(validate's own threshold: at it the command reproduces the mIoU validate printed for the same maps) and 0.05 .. 0.95.
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
    p.add_argument("--out", default=None, type=str, help="write the summary as JSON")
    p.add_argument("--per_name", default=None, type=str, help="write the per-name I/U arrays as .npz")
    return p


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
