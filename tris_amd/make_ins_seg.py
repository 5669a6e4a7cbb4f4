"""Instance masks for Stage 2 from saved response maps, either from images and the weights of the IRNet edge / displacement
network (one command from Stage 1's output to a --pseudo_path):

    python -m tris_amd.make_ins_seg --cam_out_dir D --irn_weights_name W --voc12_root IMG --ins_seg_out_dir O --train_list names.json

or from that network's outputs saved by another run:

    python -m tris_amd.make_ins_seg --cam_out_dir D --irn_out_dir E --ins_seg_out_dir O --train_list names.json

For every name of the list (what validate_same_sentence(save_cam=True) writes as {dataset}_train_names.json):
  D/{name}.npy   the response map validate_same_sentence saved (float32 [H,W], the image's own size)
  W              a state dict of IRNet's EdgeDisplacement (what train_irn.py saves, or canonical names only: tris_amd.irn_net)
  IMG/...        the image of the name: its id is name.split('_')[-1] (IRNet/voc12/dataloader.py:319-324)
  E/{name}.npz   `edge` [h,w] and `dp` [2,h,w] as EdgeDisplacement.forward returns them, h = (H-1)//4 + 1
  O/{name}.npy   the reference's dict {'score', 'mask', 'class', 'cam'} (IRNet/step_refer/make_ins_seg_labels.py:160-163)
O is then a --pseudo_path for tris_amd.train_stage2.  The argument names are those of IRNet/run_sample_refer.py.
"""
import argparse
import json
import os

import numpy as np


def get_parser():
    p = argparse.ArgumentParser(description="IRNet instance-mask synthesis on the MI355X")
    p.add_argument("--cam_out_dir", required=True)
    p.add_argument("--irn_out_dir", default=None, help="saved edge / displacement outputs (E/{name}.npz)")
    p.add_argument("--irn_weights_name", default=None, help="state dict of the edge / displacement network: run it on the images")
    p.add_argument("--voc12_root", default=None, help="image directory (with --irn_weights_name)")
    p.add_argument("--ins_seg_out_dir", required=True)
    p.add_argument("--train_list", required=True, help="JSON list of names")
    p.add_argument("--beta", default=10, type=int)
    p.add_argument("--exp_times", default=8, type=int)
    p.add_argument("--ins_seg_bg_thres", default=0.25, type=float)
    return p


def check_sources(args):
    """exactly one of --irn_out_dir and --irn_weights_name; the weights need the image directory"""
    if (args.irn_out_dir is None) == (args.irn_weights_name is None):
        raise ValueError("give exactly one of --irn_out_dir (saved edge / displacement outputs) and --irn_weights_name "
                         "(run the network on the images of --voc12_root)")
    if args.irn_weights_name is not None and args.voc12_root is None:
        raise ValueError("--irn_weights_name needs --voc12_root, the image directory")


def image_id(name):
    return name.split('_')[-1]


def image_file(name, voc12_root):
    """the reference's rule (IRNet/voc12/dataloader.py:313-324): the id is the last '_' field of the name; COCO file names, or
    {id}.jpg when the root's path contains 'referit'"""
    img_id = image_id(name)
    if 'referit' in voc12_root:
        return os.path.join(voc12_root, f'{img_id}.jpg')
    return os.path.join(voc12_root, f'COCO_train2014_{str(img_id).zfill(12)}.jpg')


def load_image(path):
    """uint8 [H,W,3]; a grey image becomes three equal channels (dataloader.py:328-330)"""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im if im.mode in ("L", "RGB") else im.convert("RGB"))
    if a.ndim == 2:
        a = np.stack([a, a, a], axis=2)
    return np.ascontiguousarray(a[:, :, :3], dtype=np.uint8)


def load_network(weights):
    import torch
    from .irn_net import EdgeDisplacement
    from . import ops
    if not torch.cuda.is_available():
        raise ops.NoGpuError("tris_amd.make_ins_seg runs the network on MI355X only (no GPU in this process)")
    net = EdgeDisplacement()
    net.load_state_dict(torch.load(weights, map_location="cpu"))
    return net.cuda()


def run(args, net=None):
    from . import irn
    check_sources(args)
    with open(args.train_list) as f:
        names = json.load(f)
    os.makedirs(args.ins_seg_out_dir, exist_ok=True)
    if args.irn_weights_name is not None and net is None:
        net = load_network(args.irn_weights_name)
    last = (None, None, None)     # (image id, edge, dp): the list is per referring expression, many names share an image
    for name in names:
        cam = np.asarray(np.load(os.path.join(args.cam_out_dir, name + ".npy"), allow_pickle=True), np.float32)
        H, W = cam.shape
        if net is not None:
            if last[0] != image_id(name):
                img = load_image(image_file(name, args.voc12_root))
                if img.shape[:2] != (H, W):
                    raise ValueError(f"{name}: response map {H}x{W} does not go with an image of {img.shape[0]}x{img.shape[1]}")
                last = (image_id(name),) + tuple(net(img))
            edge, dp = last[1], last[2]    # device tensors: they stay there between the network and the synthesis
        else:
            with np.load(os.path.join(args.irn_out_dir, name + ".npz")) as z:
                edge, dp = z["edge"], z["dp"]
        h, w = edge.shape
        if ((H - 1) // 4 + 1, (W - 1) // 4 + 1) != (h, w):
            raise ValueError(f"{name}: response map {H}x{W} does not go with an edge map of {h}x{w}")
        out = irn.make_ins_seg(cam, edge, dp, (H, W), beta=args.beta, exp_times=args.exp_times,
                               ins_seg_bg_thres=args.ins_seg_bg_thres)
        np.save(os.path.join(args.ins_seg_out_dir, name + ".npy"), out, allow_pickle=True)
    if net is not None:
        print(f"edge / displacement network: {net.calls} passes for {len(names)} names")
    return len(names)


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    try:
        check_sources(args)
    except ValueError as e:
        parser.error(str(e))
    n = run(args)
    print(f"wrote {n} instance-mask files to {args.ins_seg_out_dir}")


if __name__ == "__main__":
    main()
