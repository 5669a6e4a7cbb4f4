"""Restatement of IRNet's dense-CRF label pass (IRNet/step_refer/cam_to_ir_label.py:45-76, IRNet/misc/imutils.py:169-183) in numpy:
the oracle of csrc/crf.hip and tris_amd/crf.py.

What DenseCRF2D computes is published: the mean field of Kraehenbuehl & Koltun 2011 with the Gaussian filters evaluated on the
permutohedral lattice of Adams, Baek & Davis 2010.  This file writes that algorithm out; it is NOT a recording of pydensecrf,
which is installed on no machine of this project.  It is anchored to something independent of the lattice instead:
`exact_dense_crf`, the same mean field with the exact O(N^2) matrix exp(-|f_i - f_j|^2 / 2) (tests/test_crf_host.py).

Geometry (which lattice vertices a point touches, and with which barycentric weights) is float32 with one rounding per operation,
in a fixed order, so that the vertex set does not depend on who computed it; the kernel does the same and agrees bit for bit.
Values (splat, blur, slice, normalisation, softmax) are float64 here by default and float32 on request.
"""
import numpy as np

FIELD_BITS = 12                      # the packed key: d signed coordinates, 12 bits each, biased by 2048, coordinate 0 highest
FIELD_BIAS = 1 << (FIELD_BITS - 1)
GAUSS_SXY, GAUSS_W = 3.0, 3.0        # d.addPairwiseGaussian(sxy=3, compat=3)          (imutils.py:178)
BILAT_SXY, BILAT_SRGB, BILAT_W = 50.0, 5.0, 10.0   # d.addPairwiseBilateral(sxy=50, srgb=5, compat=10) (imutils.py:179)


# ------------------------------------------------------------------------------------------------------------------ features
def feature_tables(H, W, sxy, srgb=None):
    """the tables the host builds once, float32: x / sxy, y / sxy, v / srgb"""
    tx = np.arange(W, dtype=np.float32) / np.float32(sxy)
    ty = np.arange(H, dtype=np.float32) / np.float32(sxy)
    tc = None if srgb is None else np.arange(256, dtype=np.float32) / np.float32(srgb)
    return tx, ty, tc


def gaussian_features(H, W, sxy=GAUSS_SXY):
    tx, ty, _ = feature_tables(H, W, sxy)
    f = np.empty((H, W, 2), np.float32)
    f[..., 0] = tx[None, :]
    f[..., 1] = ty[:, None]
    return f.reshape(-1, 2)


def bilateral_features(img, sxy=BILAT_SXY, srgb=BILAT_SRGB):
    H, W = img.shape[:2]
    tx, ty, tc = feature_tables(H, W, sxy, srgb)
    f = np.empty((H, W, 5), np.float32)
    f[..., 0] = tx[None, :]
    f[..., 1] = ty[:, None]
    f[..., 2:] = tc[img]
    return f.reshape(-1, 5)


def scale_table(d):
    """scale[i] = sqrt(2/3) (d+1) / sqrt((i+1)(i+2)), in double"""
    i = np.arange(d, dtype=np.float64)
    return np.sqrt(2.0 / 3.0) * (d + 1) / np.sqrt((i + 1) * (i + 2))


def roundf(x):
    """C's roundf on float32 values (half away from zero): floor(|x| + 0.5) in float64 on the float32 value, sign restored.
    |x| + 0.5 is exact in float64 for every float32 x, so this is the exact function."""
    x64 = np.asarray(x).astype(np.float64)
    return (np.sign(x64) * np.floor(np.abs(x64) + 0.5)).astype(np.asarray(x).dtype)


# ------------------------------------------------------------------------------------------------------------------- lattice
class Lattice:
    """N points in d dimensions on the permutohedral lattice.
    rank [N,d+1] int, keys [N,d+1,d] int (vertex r of point p), bary [N,d+1] (geometry dtype), packed [N,d+1] int64,
    uniq [M] sorted packed keys, inv [N,d+1] index into uniq, nbr [d+1,2,M] int32 (-1: absent)"""


def pack(keys):
    """[..., d] int coordinates -> int64; every coordinate must fit the signed 12-bit field"""
    keys = np.asarray(keys, np.int64)
    assert keys.min() >= -FIELD_BIAS and keys.max() < FIELD_BIAS, "coordinate outside the packed field"
    out = np.zeros(keys.shape[:-1], np.int64)
    for k in range(keys.shape[-1]):
        out = (out << FIELD_BITS) | (keys[..., k] + FIELD_BIAS)
    return out


def unpack(packed, d):
    packed = np.asarray(packed, np.int64)
    out = np.empty(packed.shape + (d,), np.int64)
    for k in range(d - 1, -1, -1):
        out[..., k] = (packed & ((1 << FIELD_BITS) - 1)) - FIELD_BIAS
        packed = packed >> FIELD_BITS
    return out


def lattice_points(features, geometry_dtype=np.float32):
    """-> (rank [N,d+1] after correction, keys [N,d+1,d], bary [N,d+1]); one rounding per operation in geometry_dtype"""
    T = np.dtype(geometry_dtype).type
    f = np.asarray(features).astype(T)
    N, d = f.shape
    d1 = d + 1
    cf = f * scale_table(d).astype(T)[None, :]
    E = np.zeros((N, d1), T)
    sm = np.zeros(N, T)
    for j in range(d, 0, -1):
        E[:, j] = sm - T(j) * cf[:, j - 1]
        sm = sm + cf[:, j - 1]
    E[:, 0] = sm
    rd = roundf(E / T(d1))
    rem0 = rd * T(d1)
    S = rd.astype(np.int64).sum(1)
    diff = E - rem0
    rank = np.zeros((N, d1), np.int64)
    for i in range(d1):
        for j in range(i + 1, d1):
            lt = diff[:, i] < diff[:, j]
            rank[:, i] += lt
            rank[:, j] += ~lt
    pos, neg = (S > 0)[:, None], (S < 0)[:, None]
    Sc = S[:, None]
    wrap_p = pos & (rank >= d1 - Sc)
    wrap_n = neg & (rank < -Sc)
    rem0 = rem0 + np.where(wrap_n, T(d1), T(0)) - np.where(wrap_p, T(d1), T(0))
    rank = rank + Sc + np.where(wrap_n, d1, 0) - np.where(wrap_p, d1, 0)
    b = np.zeros((N, d + 2), T)
    rows = np.arange(N)
    for i in range(d1):
        v = (E[:, i] - rem0[:, i]) / T(d1)
        # (a rank outside [0, d] would be a bug; the clip only keeps the fancy index legal so that the test can report it)
        lo = np.clip(d - rank[:, i], 0, d + 1)
        hi = np.clip(d1 - rank[:, i], 0, d + 1)
        b[rows, lo] = b[rows, lo] + v
        b[rows, hi] = b[rows, hi] - v
    b[:, 0] = b[:, 0] + (T(1) + b[:, d1])
    r0 = rem0.astype(np.int64)
    keys = np.empty((N, d1, d), np.int64)
    for r in range(d1):
        canon = np.where(rank[:, :d] <= d - r, r, r - d1)
        keys[:, r, :] = r0[:, :d] + canon
    return rank, keys, b[:, :d1].copy()


def neighbours(uniq, d):
    """[d+1, 2, M] int32: index in the sorted keys of n1 / n2 along every axis, -1 where that vertex does not exist"""
    M = len(uniq)
    keys = unpack(uniq, d)
    out = np.full((d + 1, 2, M), -1, np.int32)
    for j in range(d + 1):
        for s, sign in enumerate((-1, 1)):
            n = keys + sign
            if j < d:
                n[:, j] -= sign * (d + 1)
            ok = (n >= -FIELD_BIAS).all(1) & (n < FIELD_BIAS).all(1)
            q = pack(np.clip(n, -FIELD_BIAS, FIELD_BIAS - 1))
            at = np.minimum(np.searchsorted(uniq, q), M - 1)
            out[j, s] = np.where(ok & (uniq[at] == q), at, -1)
    return out


def lattice(features, geometry_dtype=np.float32):
    L = Lattice()
    f = np.asarray(features)
    L.N, L.d = f.shape
    L.rank, L.keys, L.bary = lattice_points(f, geometry_dtype)
    L.packed = pack(L.keys)
    L.uniq, inv = np.unique(L.packed.ravel(), return_inverse=True)
    L.inv = inv.reshape(L.N, L.d + 1)
    L.M = len(L.uniq)
    L.nbr = neighbours(L.uniq, L.d)
    return L


def filter(L, x, norm=None, value_dtype=np.float64):
    """splat, blur along the d+1 axes in order, slice; x [N,C] (or [N]) -> the same shape.  norm [N]: norm * K(norm * x)"""
    V = np.dtype(value_dtype).type
    x = np.asarray(x)
    flat = x.ndim == 1
    xv = x.reshape(L.N, -1).astype(V)
    w = L.bary.astype(V)
    if norm is not None:
        nv = np.asarray(norm).astype(V)[:, None]
        xv = xv * nv
    C = xv.shape[1]
    d1 = L.d + 1
    val = np.zeros((L.M, C), V)
    # in (point, r) order: the order of the kernel's per-vertex lists
    np.add.at(val, L.inv.ravel(), (w[:, :, None] * xv[:, None, :]).reshape(-1, C))
    zero = np.zeros((1, C), V)
    for j in range(d1):
        old = np.concatenate([val, zero])          # index -1 reads the zero row
        val = val + V(0.5) * (old[L.nbr[j, 0]] + old[L.nbr[j, 1]])
    alpha = V(1.0 / (1.0 + 2.0 ** -L.d))
    out = np.zeros((L.N, C), V)
    for r in range(d1):
        out = out + w[:, r, None] * val[L.inv[:, r]]
    out = alpha * out
    if norm is not None:
        out = out * nv
    return out[:, 0] if flat else out


def sym_norm(L, value_dtype=np.float64):
    """1 / sqrt(K 1 + 1e-20)"""
    V = np.dtype(value_dtype).type
    return (V(1) / np.sqrt(filter(L, np.ones(L.N, V), None, value_dtype) + V(1e-20))).astype(V)


# ---------------------------------------------------------------------------------------------------------------- mean field
def unary_from_labels(labels, n_labels=2, gt_prob=0.7):
    """pydensecrf.utils.unary_from_labels(zero_unsure=False): U [n_labels, N] float32"""
    lab = np.asarray(labels).ravel()
    e_same = np.float32(-np.log(gt_prob))
    e_diff = np.float32(-np.log((1.0 - gt_prob) / (n_labels - 1)))
    U = np.full((n_labels, lab.size), e_diff, np.float32)
    U[lab, np.arange(lab.size)] = e_same
    return U


def softmax_neg(a):
    """softmax over axis 0 with the maximum subtracted"""
    a = a - a.max(0, keepdims=True)
    e = np.exp(a)
    return e / e.sum(0, keepdims=True)


def mean_field(U, terms, t=10, value_dtype=np.float64):
    """U [L,N]; terms: [(weight, apply)] with apply(Q [N,L]) -> [N,L].  -> Q [L,N]"""
    V = np.dtype(value_dtype).type
    U = U.astype(V)
    Q = softmax_neg(-U)
    for _ in range(t):
        a = -U
        for w, apply in terms:
            a = a + V(w) * apply(np.ascontiguousarray(Q.T)).T
        Q = softmax_neg(a)
    return Q


class Lattices:
    """both lattices of an image and their norms: they depend on the image alone"""

    def __init__(self, img, value_dtype=np.float64, geometry_dtype=np.float32):
        img = np.asarray(img, np.uint8)
        self.H, self.W = img.shape[:2]
        self.value_dtype = value_dtype
        self.gauss = lattice(gaussian_features(self.H, self.W), geometry_dtype)
        self.bilat = lattice(bilateral_features(img), geometry_dtype)
        self.norm_g = sym_norm(self.gauss, value_dtype)
        self.norm_b = sym_norm(self.bilat, value_dtype)

    def terms(self):
        V = self.value_dtype
        return [(GAUSS_W, lambda q: filter(self.gauss, q, self.norm_g, V)),
                (BILAT_W, lambda q: filter(self.bilat, q, self.norm_b, V))]


def dense_crf(img, labels, value_dtype=np.float64, t=10, n_labels=2, gt_prob=0.7, lattices=None, return_q=False):
    """imutils.crf_inference_label: -> arg-max label [H,W] (and Q [n_labels,H,W])"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    lat = lattices if lattices is not None else Lattices(img, value_dtype)
    Q = mean_field(unary_from_labels(labels, n_labels, gt_prob), lat.terms(), t, value_dtype).reshape(n_labels, H, W)
    pred = np.argmax(Q, axis=0)
    return (pred, Q) if return_q else pred


def exact_kernel(features):
    f = np.asarray(features, np.float64)
    sq = (f * f).sum(1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (f @ f.T), 0.0)
    return np.exp(-0.5 * d2)


def exact_sym_filter(features):
    """-> apply(x) = norm * K(norm * x) with the exact K = exp(-|f_i - f_j|^2 / 2) and norm = 1 / sqrt(K 1 + 1e-20); small N"""
    K = exact_kernel(features)
    norm = 1.0 / np.sqrt(K.sum(1) + 1e-20)
    Kn = norm[:, None] * K * norm[None, :]
    return lambda x: Kn @ np.asarray(x, np.float64)


def exact_dense_crf(img, labels, t=10, n_labels=2, gt_prob=0.7, return_q=False, terms=None):
    """the same mean field with the exact Gaussian matrices instead of the lattice (O(N^2): small images only)"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    if terms is None:
        terms = exact_terms(img)
    Q = mean_field(unary_from_labels(labels, n_labels, gt_prob), terms, t, np.float64).reshape(n_labels, H, W)
    pred = np.argmax(Q, axis=0)
    return (pred, Q) if return_q else pred


def exact_terms(img):
    H, W = img.shape[:2]
    return [(GAUSS_W, exact_sym_filter(gaussian_features(H, W))), (BILAT_W, exact_sym_filter(bilateral_features(img)))]


# ----------------------------------------------------------------------------------------------------------- cam_to_ir_label
def initial_labels(cam, thr):
    """cam_to_ir_label.py:51-52, :61-62: cams[cams < 0] = 0, argmax of [thr, cam] -- a tie gives 0"""
    c = np.asarray(cam, np.float32).copy()
    c[c < 0] = 0
    return (c > np.float32(thr)).astype(np.int64)


def combine(fg_pred, bg_pred):
    """cam_to_ir_label.py:72-74"""
    conf = np.asarray(fg_pred).astype(np.int64).copy()
    conf[fg_pred == 0] = 255
    conf[bg_pred + fg_pred == 0] = 0
    return conf.astype(np.uint8)


def ir_label(img, cam, conf_fg_thres=0.3, conf_bg_thres=0.1, t=10, gt_prob=0.7, value_dtype=np.float64, lattices=None,
             crf=None, return_q=False):
    """-> uint8 [H,W] (and Q [2 CRFs, 2 labels, H, W]); crf: the inference to use (default: the lattice one)"""
    img = np.asarray(img, np.uint8)
    if crf is None:
        lat = lattices if lattices is not None else Lattices(img, value_dtype)

        def crf(im, lab):
            return dense_crf(im, lab, value_dtype, t=t, gt_prob=gt_prob, lattices=lat, return_q=True)
    preds, qs = [], []
    for thr in (conf_fg_thres, conf_bg_thres):
        pred, q = crf(img, initial_labels(cam, thr))
        preds.append(pred)
        qs.append(q)
    conf = combine(preds[0], preds[1])
    return (conf, np.stack(qs)) if return_q else conf


# -------------------------------------------------------------------------------------------------------------------- scenes
def _scene(seed, H, W, grey=False, ties=False):
    """a smooth background, two flat-coloured regions, Gaussian pixel noise (sigma 6) and a noisy bump as the map"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = yy / max(H - 1, 1), xx / max(W - 1, 1)
    base = np.stack([90 + 60 * u + 30 * v, 120 + 50 * np.sin(3 * v), 150 - 70 * u * v], 2)
    a = (u > 0.2) & (u < 0.75) & (v > 0.15) & (v < 0.55)                 # the object
    b = ((u - 0.6) ** 2 + (v - 0.8) ** 2) < 0.02                         # a distractor of another colour
    base[a] = (200, 60, 50)
    base[b] = (40, 180, 90)
    if grey:
        base = np.repeat(base.mean(2, keepdims=True), 3, axis=2)
    img = np.clip(base + rng.normal(0, 6, base.shape if not grey else base.shape[:2] + (1,)), 0, 255).astype(np.uint8)
    bump = np.exp(-(((u - 0.48) / 0.3) ** 2 + ((v - 0.36) / 0.25) ** 2))
    cam = (0.62 * bump + rng.normal(0, 0.09, (H, W))).astype(np.float32)     # noisy: negative in the far background
    if ties:
        cam[::3, ::4] = np.float32(0.3)          # exactly the thresholds: strict > leaves them at label 0
        cam[1::3, 1::4] = np.float32(0.1)
        cam[2::5, 2::3] = np.float32(-0.25)
    return img, cam


def scenes():
    """{name: (img uint8 [H,W,3], cam float32 [H,W])}, deterministic"""
    out = {
        "s17x23": _scene(1, 17, 23),
        "s48x64": _scene(2, 48, 64),
        "s96x128": _scene(3, 96, 128),
        "s1x1": _scene(4, 1, 1),
        "s1x40": _scene(5, 1, 40),
        "grey33x40": _scene(6, 33, 40, grey=True),
        "ties31x37": _scene(7, 31, 37, ties=True),
    }
    return out


def anchor_case():
    """the 24x32 noisy image and the uniform-random signal of the filter anchor"""
    img, _ = _scene(11, 24, 32)
    x = np.random.default_rng(12).random(24 * 32)
    return img, x
