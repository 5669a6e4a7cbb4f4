"""IRNet's dense-CRF label pass on the MI355X (csrc/crf.hip): what IRNet/step_refer/cam_to_ir_label.py:45-76 does with
crf_inference_label (IRNet/misc/imutils.py:169-183) on pydensecrf.  DESIGN.md section 14 states the algorithm: the mean field of
Kraehenbuehl & Koltun 2011, both Potts terms filtered on the permutohedral lattice of Adams, Baek & Davis 2010.

The two lattices depend on the image alone: DenseCrfLattices builds them once, and every name of that image shares them.  The two
inferences of a name (foreground and background threshold) run as the four channels of one filter pass.

    lat = DenseCrfLattices(img_u8)                 # uint8 [H,W,3]
    conf = ir_label(cam, lat)                      # uint8 [H,W] on the device: 0 background, 1 object, 255 unsure

Supported size: every vertex coordinate must fit a signed 12-bit field of the packed key (check_size refuses an image by name
otherwise); images up to 2048 x 2048 fit.  There is no CPU path: without a GPU these raise ops.NoGpuError.
"""
import numpy as np

GAUSS_SXY, GAUSS_W = 3.0, 3.0                          # imutils.py:178
BILAT_SXY, BILAT_SRGB, BILAT_W = 50.0, 5.0, 10.0       # imutils.py:179
FIELD_LIMIT = (1 << 11) - 1                            # TRIS_CRF_FIELD_BITS = 12


def scale_table(d):
    """scale[i] = sqrt(2/3) (d+1) / sqrt((i+1)(i+2)), in double"""
    i = np.arange(d, dtype=np.float64)
    return np.sqrt(2.0 / 3.0) * (d + 1) / np.sqrt((i + 1) * (i + 2))


def feature_tables(H, W, sxy, srgb=None):
    """the float32 tables the kernel looks up: x / sxy, y / sxy, v / srgb"""
    tx = np.arange(W, dtype=np.float32) / np.float32(sxy)
    ty = np.arange(H, dtype=np.float32) / np.float32(sxy)
    tc = None if srgb is None else np.arange(256, dtype=np.float32) / np.float32(srgb)
    return tx, ty, tc


def coordinate_bound(feature_max):
    """an upper bound of |coordinate| over the vertices of points with features in [0, feature_max[i]] and over the neighbours
    the blur looks up: the elevated point is E[0] = sum cf, E[j] = sum_{i >= j} cf[i] - j cf[j-1] with cf = f scale >= 0; a
    vertex is within (d+1)/2 + (d+1) + d of it and a neighbour d further"""
    d = len(feature_max)
    cf = np.asarray(feature_max, np.float64) * scale_table(d)
    e = max([cf.sum()] + [max(cf[j:].sum(), j * cf[j - 1]) for j in range(1, d + 1)])
    return int(np.ceil(e)) + 4 * (d + 1)


def check_size(H, W, what="image"):
    """refuse an image whose lattice coordinates could leave the packed key's fields"""
    if H < 1 or W < 1:
        raise ValueError(f"{what}: empty image {H}x{W}")
    g = coordinate_bound([(W - 1) / GAUSS_SXY, (H - 1) / GAUSS_SXY])
    b = coordinate_bound([(W - 1) / BILAT_SXY, (H - 1) / BILAT_SXY] + [255 / BILAT_SRGB] * 3)
    if max(g, b) > FIELD_LIMIT or 6 * H * W >= 2 ** 31:
        raise ValueError(f"{what}: {H}x{W} is too large for the dense-CRF pass: lattice coordinates up to {max(g, b)} do not fit "
                         f"the packed key's signed 12-bit fields (limit {FIELD_LIMIT}; images up to 2048x2048 fit)")


class _Lattice:
    """one permutohedral lattice on the device: bary [N,d+1], inv [N,d+1] (vertex of every (pixel, r)), uniq [M] sorted packed
    keys, nbr [d+1,2,M], the per-vertex lists (order, off), norm [N] = 1 / sqrt(K 1 + 1e-20)"""

    def __init__(self, d, keys, bary):
        import torch
        from . import ops
        self.d, self.N, self.bary, self.keys = d, keys.shape[0], bary, keys
        self.uniq, inv = torch.unique(keys.reshape(-1), sorted=True, return_inverse=True)
        self.M = int(self.uniq.numel())                     # (the one size read-back of this lattice)
        self.nbr = ops.crf_neighbours(self.uniq, d)
        self.inv = inv.to(torch.int32).reshape(self.N, d + 1)
        # CSR by vertex: a stable sort keeps every vertex's (pixel, r) pairs ascending, the order splat sums them in
        self.order = torch.sort(inv, stable=True).indices.to(torch.int32)
        self.off = torch.zeros(self.M + 1, dtype=torch.int32, device=keys.device)
        self.off[1:] = torch.cumsum(torch.bincount(inv, minlength=self.M), 0)
        self.norm = None
        ones = torch.ones(self.N, 1, dtype=torch.float32, device=keys.device)
        self.norm = ops.crf_norm(self.filter(ones, normalised=False).reshape(-1))

    def filter(self, x, normalised=True):
        """x [N,C] -> norm * K(norm * x), or plain K(x)"""
        from . import ops
        return ops.crf_filter(x, self.d, self.bary, self.inv, self.order, self.off, self.nbr, self.norm if normalised else None)


class DenseCrfLattices:
    """both lattices of an image (Gaussian: (x/3, y/3); bilateral: (x/50, y/50, r/5, g/5, b/5)) and their norms, built once"""
    builds = 0          # how many were built in this process (the command's closing line)

    def __init__(self, img_u8):
        import torch
        from . import ops
        if not torch.cuda.is_available():
            raise ops.NoGpuError("tris_amd.crf runs on MI355X only (no GPU in this process); there is no CPU fallback")
        img = torch.as_tensor(np.ascontiguousarray(img_u8) if isinstance(img_u8, np.ndarray) else img_u8)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"DenseCrfLattices: expected a uint8 [H,W,3] image, got {img.dtype} {tuple(img.shape)}")
        self.H, self.W = int(img.shape[0]), int(img.shape[1])
        check_size(self.H, self.W)
        img = img.cuda().contiguous()

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
        tx, ty, _ = feature_tables(self.H, self.W, GAUSS_SXY)
        self.gauss = _Lattice(2, *ops.crf_lattice_points(None, dev(tx), dev(ty), None, dev(scale_table(2)), self.H, self.W))
        tx, ty, tc = feature_tables(self.H, self.W, BILAT_SXY, BILAT_SRGB)
        self.bilat = _Lattice(5, *ops.crf_lattice_points(img, dev(tx), dev(ty), dev(tc), dev(scale_table(5)), self.H, self.W))
        DenseCrfLattices.builds += 1


def _energies(gt_prob, n_labels=2):
    """unary_from_labels(zero_unsure=False): the two float32 energies"""
    return float(np.float32(-np.log(gt_prob))), float(np.float32(-np.log((1.0 - gt_prob) / (n_labels - 1))))


def _mean_field(U, Q, lattices, t):
    """t times Q = softmax(-U + 3 norm K_g(norm Q) + 10 norm K_b(norm Q)); U, Q [N,R,2]"""
    from . import ops
    N = U.shape[0]
    for _ in range(t):
        flat = Q.reshape(N, -1)
        g = lattices.gauss.filter(flat).view_as(U)
        b = lattices.bilat.filter(flat).view_as(U)
        Q = ops.crf_update(U, g, b, GAUSS_W, BILAT_W)
    return Q


def ir_label(cam, lattices, conf_fg_thres=0.3, conf_bg_thres=0.1, t=10, gt_prob=0.7, return_q=False):
    """cam float32 [H,W] (numpy or tensor) -> uint8 [H,W] on the device, what cam_to_ir_label.py:76 writes; with return_q also
    the final Q [2 CRFs (fg, bg threshold), 2 labels, H, W]"""
    import torch
    from . import ops
    if not torch.cuda.is_available():
        raise ops.NoGpuError("tris_amd.crf runs on MI355X only (no GPU in this process); there is no CPU fallback")
    cam = torch.as_tensor(cam)
    H, W = lattices.H, lattices.W
    if tuple(cam.shape) != (H, W):
        raise ValueError(f"response map {tuple(cam.shape)} does not go with an image of {H}x{W}")
    cam = cam.to(device="cuda", dtype=torch.float32).contiguous()
    U, Q = ops.crf_unary_cam(cam, conf_fg_thres, conf_bg_thres, *_energies(gt_prob))
    Q = _mean_field(U, Q, lattices, int(t))
    conf = ops.crf_combine(Q).view(H, W)
    if return_q:
        return conf, Q.permute(1, 2, 0).reshape(2, 2, H, W).contiguous()
    return conf


def crf_inference_label(img, labels, t=10, n_labels=2, gt_prob=0.7, lattices=None):
    """imutils.crf_inference_label for callers that have labels instead of a map: img uint8 [H,W,3], labels [H,W] of 0 / 1 ->
    the arg-max label int64 [H,W] on the device.  lattices: the image's DenseCrfLattices, when the caller keeps them."""
    import torch
    from . import ops
    if n_labels != 2:
        raise NotImplementedError(f"n_labels={n_labels}: the referring pipeline has one object and the background "
                                  "(cam_to_ir_label.py:58-63 passes n_labels = 2), and the kernels keep the two labels of a "
                                  "pixel in one register pair; more labels are not built")
    if not torch.cuda.is_available():
        raise ops.NoGpuError("tris_amd.crf runs on MI355X only (no GPU in this process); there is no CPU fallback")
    if lattices is None:
        lattices = DenseCrfLattices(img)
    H, W = lattices.H, lattices.W
    labels = torch.as_tensor(labels)
    if tuple(labels.shape) != (H, W):
        raise ValueError(f"labels {tuple(labels.shape)} do not go with an image of {H}x{W}")
    if int(labels.min()) < 0 or int(labels.max()) > 1:
        raise ValueError("labels must be 0 or 1")
    lab = labels.to(device="cuda", dtype=torch.uint8).reshape(1, H * W).contiguous()
    U, Q = ops.crf_unary_labels(lab, *_energies(gt_prob))
    Q = _mean_field(U, Q, lattices, int(t))
    return (Q[:, 0, 1] > Q[:, 0, 0]).to(torch.int64).view(H, W)      # np.argmax: the first on a tie
