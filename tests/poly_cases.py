"""Polygons shared by tests/test_poly_host.py and tests/test_gpu_poly.py, and the oracle both compare with: the unchanged
tris_amd/dataset/cocomask.py."""
import numpy as np

from tris_amd.dataset import cocomask


def oracle_mask(xy, h, w):
    """uint8 [h,w] of one polygon, as REFER.getMask forms it"""
    return cocomask.decode(cocomask.frPyObjects([list(xy)], h, w))[:, :, 0]


def merge_zero_runs(a):
    """run lengths with zero-length runs -> the counts maskApi.c leaves (a zero run joins its two neighbours)"""
    a = [int(v) for v in a]
    out, j = [a[0]], 1
    while j < len(a):
        if a[j] > 0:
            out.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                out[-1] += a[j]
                j += 1
    return out


def random_family(n, seed):
    """n polygons (xy, h, w): canvases 1x1 .. 39x39, 1-8 vertices; real, integer and out-of-frame (negative) coordinates"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = int(rng.randint(1, 40)), int(rng.randint(1, 40))
        k = int(rng.randint(1, 9))
        kind = i % 3
        if kind == 0:
            pts = rng.uniform(0, 1, (k, 2)) * [w, h]
        elif kind == 1:
            pts = np.stack([rng.randint(0, w + 1, k), rng.randint(0, h + 1, k)], 1).astype(np.float64)
        else:
            pts = rng.uniform(-0.6, 1.6, (k, 2)) * [w, h]
        if i % 7 == 0:
            pts = pts.round(2)          # (annotation files carry two decimals)
        out.append((pts.reshape(-1).tolist(), h, w))
    return out


def named_cases():
    """(name, xy, h, w)"""
    return [
        ("one vertex", [3.2, 4.1], 9, 7),
        ("two vertices", [1.0, 1.0, 6.5, 4.3], 9, 7),
        ("two vertices steep", [2.0, 0.5, 3.1, 8.0], 9, 7),
        ("repeated vertices", [1, 1, 1, 1, 6, 2, 6, 2, 3, 7, 3, 7], 9, 8),
        ("rectangle on all four borders", [0, 0, 8, 0, 8, 6, 0, 6], 6, 8),
        ("rectangle inside", [2, 1, 5, 1, 5, 4, 2, 4], 6, 8),
        ("clips to yc == h", [1, 2, 5, 2, 5, 9.7, 1, 9.4], 6, 8),
        ("below the canvas", [1, 7, 5, 7, 5, 12, 1, 12], 6, 8),
        ("all negative", [-5, -5, -1, -5, -1, -1, -5, -1], 6, 8),
        ("right of the canvas", [9, 1, 14, 1, 14, 5, 9, 5], 6, 8),
        ("bow-tie", [1, 1, 8, 8, 8, 1, 1, 8], 10, 10),
        ("h*w not a multiple of 32", [0.5, 0.5, 4.5, 1.0, 3.0, 6.5], 7, 5),
        ("1x1 covered", [0, 0, 1, 0, 1, 1, 0, 1], 1, 1),
        ("1x1 missed", [0.6, 0.6, 0.9, 0.6, 0.9, 0.9], 1, 1),
        ("one column", [0, 0, 1, 0, 1, 17, 0, 17], 17, 1),
        ("one row", [0, 0, 23, 0, 23, 1, 0, 1], 1, 23),
    ]


def all_cases(n_random, seed):
    return [(f"random {i}", xy, h, w) for i, (xy, h, w) in enumerate(random_family(n_random, seed))] + named_cases()
