"""Host-side tables for the bit-exact Pillow resize kernels (`tris_resample_u8`, `tris_gather2d_u8`).

The reference resizes PIL images with torchvision's `F.resize` (dataset/transform.py:29,32; ReferDataset.py:187), i.e.
`Image.resize(..., BILINEAR)` for images and `NEAREST` for masks.  Pillow (third-party, pinned `pillow==10.0.0` in the
reference's environment.yml:103; 12.2 in this image -- same resampler) implements them as

  * BILINEAR: two separable passes (x then y) of a triangle filter whose support is stretched by the down-scale factor
    (antialiasing).  Taps are computed in double, normalised to sum 1, rounded to 22-bit fixed point; each pass
    accumulates `0.5 + sum(pixel * tap)` in int32, shifts and saturates to uint8 (src/libImaging/Resample.c:
    precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc).
  * NEAREST: an affine scale whose source coordinate is *accumulated* (`xo += a0`) in double and truncated
    (src/libImaging/Geometry.c: ImagingScaleAffine).

Only the tables are built here (a few KB per size pair, cached); the pixel work runs on the GPU.
"""
import math
from functools import lru_cache

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _bicubic(x):
    """Pillow's bicubic_filter (Resample.c; a = -0.5, support 2.0) on an array of doubles, in its order of operations"""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


FILTERS = {"bilinear": (1.0, lambda x: np.maximum(0.0, 1.0 - np.abs(x))), "bicubic": (2.0, _bicubic)}


def resample_taps_many(axes, filter="bicubic"):
    """axes: [(in_size, out_size, idx)], idx the wanted entries of that axis' coefficient table (any order, repeats allowed)
    -> [(bounds int32[n,2], kk int32[n,ksize], ksize)].  Axes with the same tap count are computed in one pass of numpy over
    their outputs (a batch has two axes per sample).  precompute_coeffs + normalize_coeffs_8bpc in double: the weights are summed
    tap by tap (the C loop's order, not numpy's pairwise sum), divided, and rounded away from zero to 22 bits."""
    base_support = FILTERS[filter][0]
    groups = {}
    for i, (n_in, n_out, _) in enumerate(axes):
        ksize = int(math.ceil(base_support * max(float(n_in) / n_out, 1.0))) * 2 + 1
        groups.setdefault(ksize, []).append(i)
    out = [None] * len(axes)
    for ksize, members in groups.items():
        for i, r in zip(members, _taps_group([axes[i] for i in members], ksize, filter)):
            out[i] = r
    return out


def _taps_group(axes, ksize, filter):
    base_support, fn = FILTERS[filter]
    idxs = [np.asarray(idx, np.int64).reshape(-1) for _, _, idx in axes]
    for (n_in, n_out, _), idx in zip(axes, idxs):
        if idx.size and (idx.min() < 0 or idx.max() >= n_out):
            raise ValueError(f"resample_taps: output index outside 0..{n_out - 1}")
    scales = [float(n_in) / n_out for n_in, n_out, _ in axes]
    counts = [idx.size for idx in idxs]
    rep = lambda vals: np.repeat(np.asarray(vals, np.float64), counts)
    scale, support = rep(scales), rep([base_support * max(sc, 1.0) for sc in scales])
    ss = rep([1.0 / max(sc, 1.0) for sc in scales])
    in_size = np.repeat(np.asarray([n_in for n_in, _, _ in axes], np.int64), counts)
    center = (np.concatenate(idxs) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    cnt = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < cnt[:, None]
    w = np.where(live, fn((x + xmin[:, None] - center[:, None] + 0.5) * ss[:, None]), 0.0)
    ww = np.zeros(center.shape[0], np.float64)
    for t in range(ksize):                   # tap by tap, as the C loop accumulates (a dead tap adds 0.0)
        ww = ww + w[:, t]
    nz = ww != 0.0
    v = w / ww[:, None] if nz.all() else np.where(nz[:, None], w / np.where(nz, ww, 1.0)[:, None], w)
    v *= float(1 << PRECISION_BITS)
    kk = np.trunc(v + np.where(v < 0, -0.5, 0.5)).astype(np.int32)      # (a dead tap's weight is 0.0 and rounds to 0)
    bounds = np.stack([xmin, cnt], axis=1).astype(np.int32)
    out, r = [], 0
    for n in counts:
        out.append((bounds[r:r + n], kk[r:r + n], ksize))
        r += n
    return out


def resample_taps(in_size, out_size, idx, filter="bicubic"):
    """one axis of resample_taps_many"""
    return resample_taps_many([(in_size, out_size, idx)], filter)[0]


@lru_cache(maxsize=4096)
def _nearest_all(in_size, out_size):
    a = float(in_size) / out_size
    steps = np.full(out_size, a, np.float64)
    steps[0] = a * 0.5
    o = np.add.accumulate(steps)
    v = np.where(o < 0.0, -1, np.trunc(o)).astype(np.int64)
    v[(v < 0) | (v >= in_size)] = -1
    return v.astype(np.int32)


def nearest_taps(in_size, out_size, idx):
    """The entries `idx` of nearest_index(in_size, out_size): Pillow's accumulated source coordinate (`xo += a0`; np.add.accumulate
    adds in sequence as the C loop does), truncated; -1 = outside."""
    return _nearest_all(in_size, out_size)[np.asarray(idx, np.int64)]


@lru_cache(maxsize=4096)
def resample_tables(in_size, out_size, filter="bilinear"):
    """-> (bounds int32[out,2], kk int32[out,ksize], ksize) of one axis; filter "bilinear" (the triangle, the default) or
    "bicubic" (Image.BICUBIC)."""
    if filter != "bilinear":
        return resample_taps(in_size, out_size, np.arange(out_size), filter)
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(v * one - 0.5) if v < 0 else int(v * one + 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


@lru_cache(maxsize=4096)
def nearest_index(in_size, out_size):
    """-> int32[out] source index per output position (-1 = outside) for Pillow's NEAREST resize."""
    a = float(in_size) / out_size
    o = a * 0.5
    idx = np.empty(out_size, np.int32)
    for x in range(out_size):
        v = -1 if o < 0.0 else int(o)
        idx[x] = v if 0 <= v < in_size else -1
        o += a
    return idx
