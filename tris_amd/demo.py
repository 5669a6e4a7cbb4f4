"""Single-image demo on MI355X -- `get_transform`, `visualize_cam`, `get_norm_cam`, `prepare_data` with the reference's names and
leading parameters (demo.py:14-68), and the command

    python -m tris_amd.demo --img figs/demo.png --text 'man on the right' --pretrain <ckpt> [--output <dir>] \
        [--size 320 --max_query_len 20 --backbone clip-RN50 --vis_out <dir>]

which writes `<vis_out or figs>/demo_({text}).png` (demo.py:99-100), the heat map of the sentence blended 0.6 / 0.4 over the
picture.  `--pretrain` is a path, or a name under `--output` as in the other scripts; `--size` is the parser's (default 384; the
reference's script fixes 320).  The work is done by tris_amd.predict.Predictor; `visualize_cam` and `get_norm_cam` are the two
modes of ops.cam_paint (csrc/overlay.hip) at identity size, so they need the GPU like every op.

Differences from the reference's script -- its quirks, not choices about numbers:
  * channel order: the reference hands the BGR array of cv2.imread to PIL as RGB and blends the figure with the picture's channels
    swapped (demo.py:51-63, 32-36).  Here the picture is RGB throughout;
  * eval mode: the reference never calls model.eval(), so its BatchNorm runs on the batch statistics of one image.  Here the model
    is in eval mode;
  * comma splitting: the reference splits --text at commas and concatenates the token rows past the text tower's context
    (demo.py:54-59), which cannot run.  Here --text is ONE expression, commas included;
  * checkpoint: the reference hard-codes 'weights/stage2_refcocog_google.pth' (demo.py:81); here --pretrain names it, the stage is
    read from the checkpoint, and a missing file or a checkpoint that leaves weights unset raises;
  * get_transform(size) resizes to (size, size); the reference's resizes to (320, 320) whatever `size` is (demo.py:22);
  * prepare_data's module-global `img_size` (demo.py:64, 75) is an appended optional parameter;
  * the figure is written with Pillow: plt.imsave of a uint8 RGB array stores the same pixels;
  * the colour table is the project's integer "jet" (tris_amd.predict.JET), NOT compared with cv2.COLORMAP_JET: cv2 is installed on
    no machine of this project.  tools/gen_golden_overlay.py records cv2's table where it can be imported; pass it as `colormap=`.
"""
import os

import numpy as np
import torch

from . import ops
from .predict import Predictor


class _Transform:
    """ToTensor + Normalize of a PIL image, after a BILINEAR resize to (size, size) when size is given"""

    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        from PIL import Image
        from .dataset.transform import IMAGENET_MEAN, IMAGENET_STD, Normalize, ToTensor
        if self.size is not None:
            img = img.resize((self.size, self.size), Image.BILINEAR)
        x, _ = ToTensor()(img, np.zeros((1, 1), np.uint8))
        return Normalize(IMAGENET_MEAN, IMAGENET_STD)(x, None)[0]


def get_transform(size=None):
    return _Transform(size)


def _device(t, dtype):
    if not torch.cuda.is_available():
        raise ops.NoGpuError("tris_amd.demo runs on MI355X only; there is no CPU fallback")
    t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.to(device="cuda", dtype=dtype).contiguous()


def visualize_cam(normalized_heatmap, original=None, root=None, colormap=None):
    """demo.py:28-39: normalized_heatmap [H,W] in [0, 1] -> uint8 [H,W,3] RGB = colormap[uint8(255 x)], blended 0.6 / 0.4 with
    `original` (uint8 [H,W,3] RGB) when given.  Returns the array, or writes it to `root`."""
    m = _device(normalized_heatmap, torch.float32)
    lut = None if colormap is None else _device(np.asarray(colormap, dtype=np.uint8), torch.uint8)
    heat = ops.cam_paint(m.reshape(1, *m.shape[-2:]), None if original is None else _device(original, torch.uint8), lut, mode="unit")[0]
    img = heat[0].cpu().numpy()
    if root is None:
        return img
    from PIL import Image
    Image.fromarray(img).save(root)


def get_norm_cam(cam):
    """demo.py:41-48: clamp at 0, (cam - min) / (max - min + 1e-5) -> numpy float32 [H,W]"""
    m = _device(cam, torch.float32)
    norm = ops.cam_paint(m.reshape(1, *m.shape[-2:]), want_norm=True)[1]
    return norm[0].cpu().numpy()


def prepare_data(img_path, text, max_length=20, img_size=320):
    """demo.py:50-68 -> (img float32 [3,img_size,img_size], word_ids int [1,max_length], h, w); RGB, `text` one expression"""
    from PIL import Image
    from .CLIP import clip
    img = Image.open(img_path).convert("RGB")
    w, h = img.size
    word_ids = clip.tokenize(text).squeeze(0)[:max_length].unsqueeze(0)
    return get_transform(size=img_size)(img), word_ids, h, w


def checkpoint_path(args):
    if args.pretrain is None:
        raise SystemExit("demo: --pretrain <checkpoint> is required (a path, or a name under --output)")
    if os.path.isfile(args.pretrain) or args.output is None:
        return args.pretrain
    return os.path.join(args.output, args.pretrain)


def main(args):
    """-> the path of the figure"""
    if args.img is None or args.text is None:
        raise SystemExit("demo: --img <picture> and --text <expression> are required")
    predictor = Predictor.from_checkpoint(checkpoint_path(args), args)
    pred = predictor.segment(args.img, [args.text])[0]
    out_dir = args.vis_out or "figs"
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"demo_({args.text}).png")
    from PIL import Image
    Image.fromarray(pred.heat.cpu().numpy()).save(path)
    print(f"{args.text!r}: point (y, x) = {pred.point}, mask pixels = {int(pred.mask.sum())}, map range = {pred.range} -> {path}")
    return path


if __name__ == "__main__":
    from .args import get_parser
    main(get_parser().parse_args())
