"""The labels IRNet's edge / displacement network trains on, from saved response maps and the images: the reference's
IRNet/step_refer/cam_to_ir_label.py on this stack (the dense-CRF pass: tris_amd.crf, csrc/crf.hip).

    python -m tris_amd.cam_to_ir_label --cam_out_dir D --voc12_root IMG --train_list names.json --ir_label_out_dir L

For every name of the list (what validate_same_sentence(save_cam=True) writes as {dataset}_train_names.json):
  D/{name}.npy   the response map validate_same_sentence saved (float32 [H,W], the image's own size)
  IMG/...        the image of the name: its id is name.split('_')[-1] (IRNet/voc12/dataloader.py:313-324)
  L/{name}.png   8-bit grey: 1 confident object, 0 confident background, 255 neither (cam_to_ir_label.py:72-76)
L is then the --ir_label_out_dir of tris_amd.train_irn.  The argument names and defaults are those of IRNet/run_sample_refer.py;
--num_workers is accepted and unused (the lattices of an image are built once on the device and shared by its names).
"""
import argparse
import json
import os

import numpy as np

from .make_ins_seg import image_file, image_id, load_image


def get_parser():
    p = argparse.ArgumentParser(description="IRNet dense-CRF labels on the MI355X")
    p.add_argument("--cam_out_dir", default="cam_mask", type=str)
    p.add_argument("--voc12_root", default='./data/train2014', type=str, help="image directory")
    p.add_argument("--train_list", default="voc12/train_aug.txt", type=str, help="JSON list of names")
    p.add_argument("--ir_label_out_dir", default="ir_label", type=str)
    p.add_argument("--conf_fg_thres", default=0.3, type=float)
    p.add_argument("--conf_bg_thres", default=0.1, type=float)
    p.add_argument("--num_workers", default=6, type=int, help="accepted, unused")
    return p


def run(args, log=print):
    import torch
    from PIL import Image
    from . import crf, ops
    if not torch.cuda.is_available():
        raise ops.NoGpuError("tris_amd.cam_to_ir_label runs on MI355X only (no GPU in this process)")
    with open(args.train_list) as f:
        names = json.load(f)
    os.makedirs(args.ir_label_out_dir, exist_ok=True)
    last = (None, None)      # (image id, lattices): the list is per referring expression, many names share an image
    builds = 0
    for name in names:
        cam_file = os.path.join(args.cam_out_dir, name + ".npy")
        if not os.path.exists(cam_file):
            raise FileNotFoundError(f"{name}: no response map {cam_file}")
        cam = np.asarray(np.load(cam_file, allow_pickle=True), np.float32)
        if cam.ndim != 2:
            raise ValueError(f"{cam_file}: expected a response map [H,W], got shape {cam.shape}")
        if last[0] != image_id(name):
            path = image_file(name, args.voc12_root)
            if not os.path.exists(path):
                raise FileNotFoundError(f"{name}: no image {path}")
            img = load_image(path)
            crf.check_size(img.shape[0], img.shape[1], path)
            last = (image_id(name), crf.DenseCrfLattices(img))
            builds += 1
        lat = last[1]
        if cam.shape != (lat.H, lat.W):
            raise ValueError(f"{cam_file}: response map {cam.shape[0]}x{cam.shape[1]} does not go with an image of {lat.H}x{lat.W} "
                             f"({image_file(name, args.voc12_root)})")
        conf = crf.ir_label(cam, lat, conf_fg_thres=args.conf_fg_thres, conf_bg_thres=args.conf_bg_thres)
        Image.fromarray(conf.cpu().numpy()).save(os.path.join(args.ir_label_out_dir, name + ".png"))
    log(f"dense-CRF lattices: {builds} builds for {len(names)} names")
    return len(names)


def main(argv=None):
    args = get_parser().parse_args(argv)
    try:
        n = run(args)
    except (FileNotFoundError, ValueError) as e:
        raise SystemExit(f"cam_to_ir_label: {e}")
    print(f"wrote {n} label files to {args.ir_label_out_dir}")


if __name__ == "__main__":
    main()
