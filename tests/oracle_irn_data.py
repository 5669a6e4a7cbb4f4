"""The item of IRNet's training dataset, restated with Pillow and numpy: what tris_amd.dataset.irn_data and csrc/irndata.hip must
equal bit for bit, and what tests/golden/g18_irn_data.npz (recorded from the reference's own ReferAffinityDataset.__getitem__ and
ReferImageDataset.__getitem__ by tools/gen_golden_irn_data.py) pins in turn.

    draw(rng, H, W, crop)            the random numbers of one item, in the order the dataset asks for them
    apply(img, label, d, crop)       the pixels: resize, normalise, flip, crop with fills, the label at a quarter
    pair_labels(reduced, radius)     the three affinity label arrays of the pairs within `radius`
Nothing here is imported by the product.
"""
import numpy as np
from PIL import Image

import oracle_irn_loss

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
SIZES = [(37, 53), (64, 48), (51, 80), (20, 90)]       # the colour images of the fixture and of the GPU tests (H, W)
GREY_SIZE = (45, 60)
BLOCK_IMAGE = 1                                        # the image with a saturated block beside an all-zero block


def synthetic_image(i, seed=18):
    """image i of the fixture: smooth plus noise; image BLOCK_IMAGE carries a 255 block beside a 0 block (bicubic overshoot clamps
    at both ends); i == len(SIZES) is the grey one (2-D)"""
    grey = i == len(SIZES)
    H, W = GREY_SIZE if grey else SIZES[i]
    rng = np.random.default_rng(seed * 100 + i)
    yy, xx = np.mgrid[0:H, 0:W]
    planes = []
    for c in range(1 if grey else 3):
        smooth = 128 + 90 * np.sin(yy / (5.0 + c) + i) * np.cos(xx / (7.0 - c) + c)
        planes.append(np.clip(smooth + rng.normal(0, 25, (H, W)), 0, 255))
    a = np.stack(planes, axis=2).astype(np.uint8)
    if i == BLOCK_IMAGE:
        a[10:30, 8:20] = 255
        a[10:30, 20:32] = 0
    return a[:, :, 0].copy() if grey else a


def synthetic_label(i, seed=18):
    """values {0, 1, 255} in blobs a few pixels wide, the image's size"""
    H, W = GREY_SIZE if i == len(SIZES) else SIZES[i]
    rng = np.random.default_rng(seed * 100 + 50 + i)
    coarse = rng.choice(np.asarray([0, 1, 255], np.uint8), size=(-(-H // 6), -(-W // 6)), p=[0.45, 0.35, 0.2])
    return np.ascontiguousarray(np.kron(coarse, np.ones((6, 6), np.uint8))[:H, :W])


# ------------------------------------------------------------------------------------------------------------------ the draw
def draw(rng, H, W, crop, rescale=(0.5, 1.5), hor_flip=True):
    """-> dict(scale, flip, target (h, w), cont (top, left), src (top, left), size (ch, cw)): one uniform number for the scale, one
    bit for the flip, then one bounded integer for the horizontal offset and one for the vertical"""
    scale = rescale[0] + rng.random() * (rescale[1] - rescale[0])
    h, w = int(np.round(H * scale)), int(np.round(W * scale))
    flip = bool(rng.getrandbits(1)) if hor_flip else False
    offs = {}
    for axis, n in (("x", w), ("y", h)):          # the width is asked for first
        k = rng.randrange(abs(n - crop) + 1)
        offs[axis] = (0, k) if n > crop else (k, 0)      # (offset in the container, offset in the image)
    return {"scale": scale, "flip": flip, "target": (h, w), "cont": (offs["y"][0], offs["x"][0]),
            "src": (offs["y"][1], offs["x"][1]), "size": (min(crop, h), min(crop, w))}


def top_left(H, W, crop):
    return {"scale": 1.0, "flip": False, "target": (H, W), "cont": (0, 0), "src": (0, 0), "size": (min(crop, H), min(crop, W))}


def from_params(p):
    """an IrnAugParams of the product in this module's form"""
    ct, cb, cl, cr, it, ib, il, ir = p.box
    return {"scale": p.scale, "flip": p.flip, "target": tuple(p.target), "cont": (ct, cl), "src": (it, il), "size": (cb - ct, cr - cl)}


def box8(d):
    (ct, cl), (it, il), (ch, cw) = d["cont"], d["src"], d["size"]
    return (ct, ct + ch, cl, cl + cw, it, it + ch, il, il + cw)


# ---------------------------------------------------------------------------------------------------------------- the pixels
def resize(a, size, resample):
    """Pillow's resize to size = (h, w); an array already of that size is returned as it is"""
    if tuple(a.shape[:2]) == tuple(size):
        return a
    return np.asarray(Image.fromarray(a).resize((size[1], size[0]), resample))


def normalise(a):
    out = np.empty(a.shape, np.float32)
    for c in range(3):
        out[..., c] = (a[..., c] / 255. - MEAN[c]) / STD[c]
    return out


def paste(a, d, crop, fill):
    (ct, cl), (it, il), (ch, cw) = d["cont"], d["src"], d["size"]
    out = np.full((crop, crop) + a.shape[2:], fill, a.dtype)
    out[ct:ct + ch, cl:cl + cw] = a[it:it + ch, il:il + cw]
    return out


def apply(img, label, d, crop):
    """img uint8 [H,W,3] or [H,W], label uint8 [H,W] or None -> (img float32 [crop,crop,3], label uint8 [crop,crop], reduced uint8
    [crop/4,crop/4]); label and reduced are None without a label"""
    a = resize(img, d["target"], Image.BICUBIC)
    if a.ndim == 2:
        a = np.stack([a, a, a], axis=2)
    a = normalise(a)
    lab = None if label is None else resize(label, d["target"], Image.NEAREST)
    if d["flip"]:
        a = np.fliplr(a)
        lab = None if lab is None else np.fliplr(lab)
    a = paste(a, d, crop, 0)
    if lab is None:
        return a, None, None
    lab = paste(lab, d, crop, 255)
    h = int(np.round(crop * 0.25))
    return a, lab, resize(lab, (h, h), Image.NEAREST)


def pair_labels(reduced, radius):
    """-> (bg, fg, neg) float32 [D, pairs]: for every source pixel of the top band and every direction within `radius` (ordered by
    ascending path length, as the reference's PathIndex orders its destinations), whether both ends are labelled (< 21) and equal
    at 0, equal above 0, or different"""
    h, w = reduced.shape
    r = radius - 1
    hs, ws = h - r, w - 2 * r
    paths = oracle_irn_loss.reference_paths(radius)
    order = [p for L in sorted({len(c) for _, c in paths}) for p in paths if len(p[1]) == L]
    a = reduced[:hs, r:r + ws].reshape(1, -1)
    b = np.stack([reduced[dy:dy + hs, r + dx:r + dx + ws].reshape(-1) for (dy, dx), _ in order])
    valid = (a < 21) & (b < 21)
    same = a == b
    return ((valid & same & (a == 0)).astype(np.float32), (valid & same & (a > 0)).astype(np.float32),
            (valid & ~same).astype(np.float32))
