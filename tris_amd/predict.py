"""Single-image inference: one picture and its sentences -> mask, pointing location and the heat-map figure of the paper, with no
dataset, annotation file or target.

    from tris_amd.predict import Predictor
    p = Predictor.from_checkpoint("weights/stage2_refcocog_google.pth", args)      # args: tris_amd.args.get_parser()
    for r in p.segment("figs/demo.png", ["man on the right", "the dog"]):
        r.mask, r.point, r.heat                                                      # device tensors; r.numpy() copies them

What runs, per image (all sentences together):
  * the picture is uploaded ONCE as uint8 and resized on the device with Pillow's BILINEAR tables (ops.resample_u8), then
    normalised through `normalize_table()` (ops.gather_normalize): `get_transform(size, train=False)` on the PIL image, bit for bit;
  * one trunk pass, one text pass and the heads per sentence (`encode_visual` + `forward_pairs`) under ops.batch_invariant(), as
    tris_amd.validate runs them: a sentence's result does not depend on the sentences it shares the call with;
  * ops.eval_post_group on a zero target (signed=True for `signed_maps` models): `cam` is the normalised map validate scores,
    `mask = cam > 1e-9` the very pixels it counts, `point` its pointing-game arg-max;
  * ops.cam_paint (csrc/overlay.hip): the presentation pass of demo.py:28-48, 94-100 -- resize, clamp, min-max, 8 bits, colour
    table, 0.6 / 0.4 blend -- for all sentences in one call, into uint8;
  * one host fetch (the K arg-max words and ranges).

The model is in eval mode and the picture is RGB throughout (see tris_amd.demo for how the reference's script differs).

The colour table `JET` is a PROJECT RULE: the published piecewise-linear "jet" written with integers so that it has no rounding
question.  It has not been compared with cv2.COLORMAP_JET (cv2 can be imported on no machine of this project); whoever has cv2's
table passes it as `colormap=` (tools/gen_golden_overlay.py records it).
"""
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import ops


def jet_table():
    """uint8 [256,3] RGB: for channel (r, g, b) with centre c = (3, 2, 1), t = 765 - 2 |4 i - 255 c|, entry = clamp((t + 1) >> 1,
    0, 255).  Dark blue (0, 0, 128) at 0, dark red (128, 0, 0) at 255."""
    i = np.arange(256, dtype=np.int64)[:, None]
    c = np.array([3, 2, 1], dtype=np.int64)[None, :]
    t = 765 - 2 * np.abs(4 * i - 255 * c)
    return np.clip((t + 1) >> 1, 0, 255).astype(np.uint8)


JET = jet_table()


@dataclass
class Prediction:
    sentence: str
    cam: torch.Tensor        # float32 [H,W]: validate's normalised map
    mask: torch.Tensor       # bool [H,W]: cam > 1e-9
    point: tuple             # (y, x): the pointing-game location
    heat: torch.Tensor       # uint8 [H,W,3] RGB: the overlay
    range: tuple             # (min, max) of the resized, clamped map the overlay was normalised with

    def numpy(self):
        """the same record with the tensors copied to the host"""
        return Prediction(self.sentence, self.cam.cpu().numpy(), self.mask.cpu().numpy(), self.point, self.heat.cpu().numpy(),
                          self.range)


def _as_u8_rgb(image, device):
    """path | PIL.Image | uint8 [H,W] / [H,W,3] array or tensor -> uint8 [H,W,3] on the device (a grey image: three equal channels)"""
    if isinstance(image, (str, os.PathLike)):
        from PIL import Image
        if not os.path.isfile(image):
            raise FileNotFoundError(f"image {os.fspath(image)!r} not found")
        image = Image.open(image)
    if hasattr(image, "convert") and hasattr(image, "mode"):                     # PIL
        image = np.asarray(image if image.mode == "RGB" else image.convert("RGB")).copy()
    t = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
    if t.dtype != torch.uint8:
        raise TypeError(f"the picture must be uint8, got {t.dtype}")
    if t.dim() == 2:
        t = t.unsqueeze(-1).expand(-1, -1, 3)
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"the picture is [H,W] or [H,W,3], got {tuple(t.shape)}")
    return t.to(device).contiguous()


class Predictor:
    def __init__(self, model, size=320, max_query_len=20, tokenizer=None, colormap=None):
        if not torch.cuda.is_available():
            raise ops.NoGpuError("tris_amd.predict runs on MI355X only; there is no CPU fallback")
        from .CLIP import clip
        from .dataset.transform import normalize_table
        self.model = model.eval()
        self.net = model.module if hasattr(model, "module") else model
        self.size, self.max_query_len = int(size), int(max_query_len)
        if self.size * self.size % 4:
            raise ValueError(f"size {size}: size * size must be a multiple of 4 (ops.gather_normalize)")
        self.tokenizer = tokenizer or clip.tokenize            # same call signature as clip.tokenize
        self.device = next(self.net.parameters()).device
        self.signed = bool(getattr(self.net, "signed_maps", False))
        lut = JET if colormap is None else np.asarray(colormap)
        if lut.shape != (256, 3) or lut.dtype != np.uint8:
            raise ValueError(f"colormap is uint8 [256,3] RGB, got {lut.dtype} {lut.shape}")
        self.colormap = torch.from_numpy(lut.copy()).to(self.device)
        self._lut = normalize_table().to(self.device)
        self._slot = torch.zeros(1, dtype=torch.int64, device=self.device)

    @classmethod
    def from_checkpoint(cls, path, args, **kw):
        """A checkpoint that holds the Stage-2 decoder (`reduced_c1.*`) builds model_stage2.TRIS, anything else model_stage1.TRIS
        (the rule of validate_referit).  Every weight comes from the file: a missing file, or a checkpoint that leaves a parameter
        of the model unset, raises -- there is no silent random initialisation."""
        import warnings
        from .CLIP import clip
        if not os.path.isfile(path):
            raise FileNotFoundError(f"checkpoint {os.fspath(path)!r} not found")
        if not torch.cuda.is_available():
            raise ops.NoGpuError("tris_amd.predict runs on MI355X only; there is no CPU fallback")
        ckpt = torch.load(path, map_location="cpu")
        sd = ckpt.get("model", ckpt)
        if any(k.startswith("reduced_c1.") for k in sd):
            from .model.model_stage2 import TRIS
        else:
            from .model.model_stage1 import TRIS
        with warnings.catch_warnings(), clip.random_init():     # the architecture only: the file supplies every weight (checked)
            warnings.simplefilter("ignore")
            model = TRIS(args).cuda()
        res = model.load_state_dict(sd, strict=False)
        if res.missing_keys:
            raise RuntimeError(f"checkpoint {os.fspath(path)!r} leaves {len(res.missing_keys)} tensors of {TRIS.__module__}.TRIS "
                               f"unset (first: {res.missing_keys[:3]})")
        kw.setdefault("size", args.size)
        kw.setdefault("max_query_len", args.max_query_len)
        return cls(model, **kw)

    def tokenize(self, sentences):
        """-> int64 [K, max_query_len] on the device: tokenizer(s)[0][:max_query_len] per sentence (ReferDataset.py:94-119)"""
        rows = [torch.as_tensor(self.tokenizer(s)).reshape(-1)[: self.max_query_len].to(torch.int64) for s in sentences]
        for s, r in zip(sentences, rows):
            if r.numel() != self.max_query_len:
                raise ValueError(f"the tokenizer gave {r.numel()} tokens for {s!r}, fewer than max_query_len = {self.max_query_len}")
        return torch.stack(rows).to(self.device)

    def preprocess(self, image):
        """-> (picture uint8 [H,W,3] on the device, model input float32 [1,3,size,size])"""
        pic = _as_u8_rgb(image, self.device)
        small = ops.resample_u8(pic, self.size, self.size)
        return pic, ops.gather_normalize(small.unsqueeze(0), self._slot, self._lut, planar=True)

    @torch.no_grad()
    def segment(self, image, sentences):
        if isinstance(sentences, str):
            sentences = [sentences]
        sentences = list(sentences)
        if not sentences:
            return []
        K = len(sentences)
        ids = self.tokenize(sentences)
        pic, x = self.preprocess(image)
        H, W = pic.shape[:2]
        self.model.eval()
        with ops.batch_invariant():
            vis = self.net.encode_visual(x)                                              # once per image
            maps = self.net.forward_pairs(vis, ids, [0] * K, self.size).contiguous()     # [K,1,S,S]
            records, cams = ops.eval_post_group(maps, torch.zeros(K, H, W, dtype=torch.uint8, device=self.device),
                                                signed=self.signed)
        heat, _, rng, _ = ops.cam_paint(maps, pic, self.colormap)
        vals = torch.cat([records[:, 2:3].to(torch.float64), rng.to(torch.float64)], 1).tolist()   # the one host fetch
        out = []
        for k, s in enumerate(sentences):
            am = int(vals[k][0])
            out.append(Prediction(s, cams[k], cams[k] > 1e-9, divmod(am, W), heat[k], (float(vals[k][1]), float(vals[k][2]))))
        return out
