"""Instance masks for Stage 2 from saved response maps and the edge / displacement outputs of the IRNet network:

    python -m tris_amd.make_ins_seg --cam_out_dir D --irn_out_dir E --ins_seg_out_dir O --train_list names.json

For every name of the list (what validate_same_sentence(save_cam=True) writes as {dataset}_train_names.json):
  D/{name}.npy   the response map validate_same_sentence saved (float32 [H,W], the image's own size)
  E/{name}.npz   `edge` [h,w] and `dp` [2,h,w] as EdgeDisplacement.forward returns them, h = (H-1)//4 + 1
  O/{name}.npy   the reference's dict {'score', 'mask', 'class', 'cam'} (IRNet/step_refer/make_ins_seg_labels.py:160-163)
O is then a --pseudo_path for tris_amd.train_stage2.  The argument names are those of IRNet/run_sample_refer.py.
"""
import argparse
import json
import os

import numpy as np


def get_parser():
    p = argparse.ArgumentParser(description="IRNet instance-mask synthesis (post-network half) on the MI355X")
    p.add_argument("--cam_out_dir", required=True)
    p.add_argument("--irn_out_dir", required=True)
    p.add_argument("--ins_seg_out_dir", required=True)
    p.add_argument("--train_list", required=True, help="JSON list of names")
    p.add_argument("--beta", default=10, type=int)
    p.add_argument("--exp_times", default=8, type=int)
    p.add_argument("--ins_seg_bg_thres", default=0.25, type=float)
    return p


def run(args):
    from . import irn
    with open(args.train_list) as f:
        names = json.load(f)
    os.makedirs(args.ins_seg_out_dir, exist_ok=True)
    for name in names:
        cam = np.asarray(np.load(os.path.join(args.cam_out_dir, name + ".npy"), allow_pickle=True), np.float32)
        with np.load(os.path.join(args.irn_out_dir, name + ".npz")) as z:
            edge, dp = z["edge"], z["dp"]
        h, w = edge.shape
        H, W = cam.shape
        if ((H - 1) // 4 + 1, (W - 1) // 4 + 1) != (h, w):
            raise ValueError(f"{name}: response map {H}x{W} does not go with an edge map of {h}x{w}")
        out = irn.make_ins_seg(cam, edge, dp, (H, W), beta=args.beta, exp_times=args.exp_times,
                               ins_seg_bg_thres=args.ins_seg_bg_thres)
        np.save(os.path.join(args.ins_seg_out_dir, name + ".npy"), out, allow_pickle=True)
    return len(names)


def main(argv=None):
    args = get_parser().parse_args(argv)
    n = run(args)
    print(f"wrote {n} instance-mask files to {args.ins_seg_out_dir}")


if __name__ == "__main__":
    main()
