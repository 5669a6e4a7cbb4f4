"""numpy fp64 restatement of tris_cam_paint_f32 (include/tris_hip.h; the reference's demo.py:28-48, 94-96) and the rule that
decides equality with it.

Sample positions.  F.interpolate(align_corners=True) -- and csrc/bilinear.h, which restates it -- DEFINE the source position of
an output index in float32: scale = float32(in - 1) / float32(out - 1), src = scale * float32(dst), i0 = int(src),
w = src - i0 (exact in float32).  These four values are part of the specification, not round-off of it, so they are formed
here in float32 too; everything after them (the two lerps, the clamp, min, max, the normalisation, the product with 255) is in
float64.

Equality.  v = n * 255 in float64.  A pixel is NEAR A STEP when round(v) >= 1 and |v - round(v)| < 2^-10: there either
neighbouring colour index is accepted; elsewhere the index, hence every heat byte, must be the oracle's.  The float32 pass makes
about ten roundings per pixel (seven in the interpolation, three in the normalisation) on values <= 1 relative to the range, i.e.
|error of n| <~ 10 * 2^-24 and |error of v| <~ 255 * 10 * 2^-24 = 1.5e-4, well under 2^-10 = 9.8e-4; pixels with v < 1 are index 0
on both sides.  Near-step pixels may be at most 2 % of a case (NEAR_CAP): the tests assert the cap itself.  norm and range are
compared at 2^-19 absolute, the same derivation with a factor of three to spare.
"""
import numpy as np

NEAR = 2.0 ** -10
NEAR_CAP = 0.02
TOL = 2.0 ** -19
MINMAX, UNIT = "minmax", "unit"


def jet_table():
    """the project's integer "jet": channel (r, g, b) with centre c = (3, 2, 1): t = 765 - 2 |4 i - 255 c|, clamp((t + 1) >> 1, 0, 255)"""
    out = np.zeros((256, 3), np.uint8)
    for i in range(256):
        for ch, c in enumerate((3, 2, 1)):
            t = 765 - 2 * abs(4 * i - 255 * c)
            out[i, ch] = min(max((t + 1) >> 1, 0), 255)
    return out


def _axis(n_in, n_out):
    """-> (i0, i1 int64 [n_out], w float64 [n_out]) with the float32 position arithmetic of csrc/bilinear.h"""
    sc = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (sc * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float64)


def upsample(m, H, W):
    """bilinear, align_corners=True: m [Sh,Sw] -> float64 [H,W]"""
    m = np.asarray(m, np.float64)
    y0, y1, wy = _axis(m.shape[0], H)
    x0, x1, wx = _axis(m.shape[1], W)
    top = m[y0][:, x0] + wx[None, :] * (m[y0][:, x1] - m[y0][:, x0])
    bot = m[y1][:, x0] + wx[None, :] * (m[y1][:, x1] - m[y1][:, x0])
    return top + wy[:, None] * (bot - top)


def paint(maps, H, W, image=None, lut=None, mode=MINMAX):
    """maps [K,Sh,Sw] -> dict: v float64 [K,H,W] (= n * 255), norm float64, index int64, heat uint8 [K,H,W,3], range float64 [K,2],
    argmax int64 [K], near bool [K,H,W]"""
    lut = jet_table() if lut is None else np.asarray(lut)
    K = len(maps)
    u = np.stack([np.maximum(upsample(m, H, W), 0.0) for m in maps]) if K else np.zeros((0, H, W))
    lo, hi = u.reshape(K, -1).min(1), u.reshape(K, -1).max(1)
    if mode == MINMAX:
        n = (u - lo[:, None, None]) / (hi - lo + np.float64(np.float32(1e-5)))[:, None, None]
    else:
        n = np.minimum(u, 1.0)
    v = n * 255.0
    idx = np.clip(v.astype(np.int64), 0, 255)
    rv = np.round(v)
    return {"v": v, "norm": n, "index": idx, "heat": blend(lut[idx], image), "range": np.stack([lo, hi], 1),
            "argmax": u.reshape(K, -1).argmax(1), "near": (rv >= 1) & (np.abs(v - rv) < NEAR), "lut": lut, "image": image}


def blend(colour, image):
    """cv2.addWeighted(colour, .6, image, .4, 0) on uint8 with round-to-nearest, in integers: (3 c + 2 p + 2) // 5"""
    if image is None:
        return colour.astype(np.uint8)
    return ((3 * colour.astype(np.int64) + 2 * np.asarray(image, np.int64) + 2) // 5).astype(np.uint8)


def near_fraction(ref):
    return float(ref["near"].mean()) if ref["near"].size else 0.0


def check_heat(heat, ref):
    """heat uint8 [K,H,W,3] against paint(): exact away from steps, either neighbouring index at a near-step pixel"""
    assert near_fraction(ref) <= NEAR_CAP, f"{near_fraction(ref):.4f} of the pixels are near a step: not a usable input"
    heat = np.asarray(heat)
    assert heat.shape == ref["heat"].shape and heat.dtype == np.uint8
    bad = (heat != ref["heat"]).any(-1)
    assert not (bad & ~ref["near"]).any(), f"{int((bad & ~ref['near']).sum())} pixels away from a step differ"
    if bad.any():                                            # near a step: the other neighbour, round(v) or round(v) - 1
        rv = np.round(ref["v"]).astype(np.int64)
        other = np.clip(np.where(ref["index"] == rv, rv - 1, rv), 0, 255)
        alt = blend(ref["lut"][other], ref["image"])
        assert not (bad & (heat != alt).any(-1)).any(), "a near-step pixel has neither neighbouring colour"


def check_all(got, ref, norm=True):
    """got = (heat, norm | None, range, argmax) as numpy"""
    heat, nrm, rng, arg = got
    print("  |range - oracle| max", np.abs(np.asarray(rng, np.float64) - ref["range"]).max(initial=0.0),
          "|norm - oracle| max", None if nrm is None else np.abs(np.asarray(nrm, np.float64) - ref["norm"]).max(initial=0.0),
          "bound", TOL)
    check_heat(heat, ref)
    assert np.abs(np.asarray(rng, np.float64) - ref["range"]).max(initial=0.0) <= TOL      # (the test maps lie in [-1, 1])
    if norm:
        assert np.abs(np.asarray(nrm, np.float64) - ref["norm"]).max(initial=0.0) <= TOL
    else:
        assert nrm is None
    assert np.array_equal(np.asarray(arg, np.int64), ref["argmax"])


# ---------------------------------------------------------------------------------------------------------- the test inputs
# (Sh, Sw, H, W, K): the smallest shapes at which the kernel can go wrong -- one pixel; one row; a partial 4-pixel group and a
# sentence boundary that is no multiple of 4; several blocks; more pixels than one pass of either grid; a non-square source that
# is down-sampled.  Maps are float32-valued in [-1, 1] (signed: the clamp matters), pictures uniform bytes.
SHAPES = [(1, 1, 1, 1, 1), (2, 2, 1, 9, 1), (2, 2, 7, 5, 2), (10, 10, 37, 50, 3), (20, 20, 333, 480, 3), (64, 48, 50, 37, 2)]


def case_maps(Sh, Sw, K, seed=0):
    return np.random.RandomState(1000 + seed).uniform(-1, 1, (K, Sh, Sw)).astype(np.float32)


def case_image(H, W, seed=0):
    return np.random.RandomState(2000 + seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def special_cases():
    """name -> (maps [K,Sh,Sw], (H, W), mode)"""
    two = np.random.RandomState(5).uniform(-1, 0.5, (1, 40, 40)).astype(np.float32)
    two.reshape(-1)[[300, 600]] = 1.0        # equal maxima in two different blocks of the range pass; the first is pixel 300
    return {
        "all_negative": (-np.abs(case_maps(10, 10, 2, 7)) - np.float32(0.125), (37, 50), MINMAX),
        "constant": (np.full((2, 10, 10), 0.75, np.float32), (37, 50), MINMAX),
        "two_maxima": (two, (40, 40), MINMAX),
        "signed": (case_maps(10, 10, 3, 8) - np.float32(0.5), (37, 50), MINMAX),
        "unit": (np.random.RandomState(9).uniform(0, 1, (2, 37, 50)).astype(np.float32), (37, 50), UNIT),
    }
