"""numpy restatement of the post-network half of IRNet's make_ins_seg_labels (IRNet/step_refer/make_ins_seg_labels.py,
IRNet/misc/indexing.py): what tris_amd/irn.py computes on the GPU, stage by stage, without scipy or skimage.

The walk is float64 in its sparse form: x T^(2^t) as 2^t gathers over the 34 search directions (both ways) and the diagonal.
The integer stages (centroids, labelling, instance map, fragments) follow the reference operation for operation.
"""
import numpy as np


# ------------------------------------------------------------------------------------------------------ search paths
def search_paths(radius=5):
    """[((dy, dx), [(y, x), ...])] from the definition: the cells of the bounding box closer than 1 to the line"""
    dirs = [(0, x) for x in range(1, radius)]
    for y in range(1, radius):
        dirs += [(y, x) for x in range(-radius + 1, radius) if x * x + y * y < radius ** 2]
    out = []
    for dy, dx in dirs:
        cells = [(y, x) for y in range(dy + 1) for x in range(min(dx, 0), max(dx, 0) + 1)
                 if (dy * x - dx * y) ** 2 / (dy * dy + dx * dx) < 1]
        out.append(((dy, dx), cells))
    return out


# ------------------------------------------------------------------------------------------- connected components
def cc_label(mask):
    """4-connected components of a 2-D mask, numbered 1.. by first pixel in raster order (skimage.measure.label with
    connectivity=1, background=0) -> (int32 labels, count)"""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    lab = np.zeros((H, W), np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(mask)):      # raster order
        if lab[y0, x0]:
            continue
        n += 1
        lab[y0, x0] = n
        stack = [(y0, x0)]
        while stack:
            y, x = stack.pop()
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < H and 0 <= xx < W and mask[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = n
                    stack.append((yy, xx))
    return lab, n


# ---------------------------------------------------------------------------------------------------- centroids
def find_centroids(dp, iterations=300):
    """float32 centroids, float64 inside a step (numpy promotes float32 - int32 to float64), one rounding to float32 per step"""
    dp = np.asarray(dp, np.float32)
    h, w = dp.shape[1:]
    cy, cx = [a.astype(np.float32) for a in np.mgrid[0:h, 0:w]]
    for _ in range(iterations):
        uy, ly = np.ceil(cy).astype(np.int32), np.floor(cy).astype(np.int32)
        ux, lx = np.ceil(cx).astype(np.int32), np.floor(cx).astype(np.int32)
        fy = cy.astype(np.float64) - ly
        fx = cx.astype(np.float64) - lx
        step = []
        for d in dp.astype(np.float64):
            step.append(d[uy, ux] * fy * fx + d[ly, ux] * (1 - fy) * fx + d[uy, lx] * fy * (1 - fx) + d[ly, lx] * (1 - fy) * (1 - fx))
        cy = (cy.astype(np.float64) + step[0]).astype(np.float32)
        cx = (cx.astype(np.float64) + step[1]).astype(np.float32)
        cy = np.clip(cy, np.float32(0), np.float32(h - 1))
        cx = np.clip(cx, np.float32(0), np.float32(w - 1))
    return np.stack([np.round(cy).astype(np.int32), np.round(cx).astype(np.int32)])


def weak_mask(dp, thres=2.5):
    dp = np.asarray(dp, np.float32)
    return np.sqrt(dp[1] ** 2 + dp[0] ** 2) < thres


def instance_map(centroids, dp, thres=2.5):
    """-> (int32 [h,w] in 0..K-1, K): the weak-region label under each centroid, ranked among the labels that occur"""
    lab, _ = cc_label(weak_mask(dp, thres))
    at = lab[centroids[0], centroids[1]]
    vals, inv = np.unique(at, return_inverse=True)
    return inv.reshape(at.shape).astype(np.int32), len(vals)


def resize_align_corners(cam, h, w):
    """F.interpolate(bilinear, align_corners=True) of a 2-D map, float64"""
    cam = np.asarray(cam, np.float64)
    H, W = cam.shape
    sy = np.arange(h) * ((H - 1) / (h - 1) if h > 1 else 0.0)
    sx = np.arange(w) * ((W - 1) / (w - 1) if w > 1 else 0.0)
    y0, x0 = np.minimum(sy.astype(int), H - 1), np.minimum(sx.astype(int), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    wy, wx = (sy - y0)[:, None], (sx - x0)[None, :]
    top = cam[y0][:, x0] * (1 - wx) + cam[y0][:, x1] * wx
    bot = cam[y1][:, x0] * (1 - wx) + cam[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


# ------------------------------------------------------------------------------------------------ affinity and walk
def affinity(edge, beta=10, radius=5):
    """float64: Wt [D,h,w] = (1 - max edge on the path to p + dir) ^ beta (0 where p + dir is outside), colsum [h,w]"""
    edge = np.asarray(edge, np.float64)
    h, w = edge.shape
    paths = search_paths(radius)
    Wt = np.zeros((len(paths), h, w))
    colsum = np.ones((h, w))
    for d, ((dy, dx), cells) in enumerate(paths):
        ys, xs = slice(0, h - dy), slice(max(0, -dx), w - max(0, dx))     # sources whose destination is inside
        if ys.stop <= 0 or xs.stop <= xs.start:
            continue
        m = np.full((ys.stop, xs.stop - xs.start), -np.inf)
        for cy, cx in cells:
            m = np.maximum(m, edge[cy:cy + ys.stop, xs.start + cx:xs.stop + cx])
        Wt[d][ys, xs] = (1 - m) ** beta
        colsum += Wt[d]
        colsum[dy:, xs.start + dx:xs.stop + dx] += Wt[d][ys, xs]
    return Wt, colsum


def _shifted(a, dy, dx):
    """out[..., y, x] = a[..., y + dy, x + dx], 0 outside"""
    h, w = a.shape[-2:]
    out = np.zeros_like(a)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def walk(x, edge, Wt, colsum, steps, radius=5):
    """float64 sparse walk: v0 = x (1 - edge); v[j] <- (v[j] + sum_d Wt[d][j] v[j+dir] + Wt[d][j-dir] v[j-dir]) / colsum[j]"""
    dirs = [d for d, _ in search_paths(radius)]
    v = np.asarray(x, np.float64) * (1 - np.asarray(edge, np.float64))
    for _ in range(steps):
        acc = v.copy()
        for d, (dy, dx) in enumerate(dirs):
            acc += Wt[d] * _shifted(v, dy, dx)
            acc += _shifted(Wt[d] * v, -dy, -dx)
        v = acc / colsum
    return v


def propagate_to_edge(x, edge, beta=10, exp_times=8):
    """x [K,h,w] -> rw [K,h,w], float64"""
    Wt, colsum = affinity(edge, beta)
    return walk(x, edge, Wt, colsum, 2 ** exp_times)


# ---------------------------------------------------------------------------------------------------------- finish
def upsample4(rw, size):
    """F.interpolate(scale_factor=4, bilinear, align_corners=False)[..., :H, :W] in the dtype of rw"""
    rw = np.asarray(rw)
    h, w = rw.shape[-2:]
    H, W = size
    t = rw.dtype.type

    def axis(n_out, n_in):
        src = np.maximum(t(0.25) * (np.arange(n_out).astype(rw.dtype) + t(0.5)) - t(0.5), t(0))
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, (src - i0).astype(rw.dtype)

    y0, y1, wy = axis(H, h)
    x0, x1, wx = axis(W, w)
    wy = wy[:, None]
    top = rw[..., y0, :][..., x0] + wx * (rw[..., y0, :][..., x1] - rw[..., y0, :][..., x0])
    bot = rw[..., y1, :][..., x0] + wx * (rw[..., y1, :][..., x1] - rw[..., y1, :][..., x0])
    return top + wy * (bot - top)


def finish(rw, size, bg_thres=0.25):
    """-> (rw_up [K,H,W] normalised by its maximum, labels int32 [H,W], gap [H,W] = top-1 minus top-2 of [bg, rows...])"""
    up = upsample4(rw, size)
    up = up / up.max()
    stack = np.concatenate([np.full((1,) + up.shape[1:], bg_thres, up.dtype), up])
    labels = np.argmax(stack, 0).astype(np.int32)
    srt = np.sort(stack, 0)
    return up, labels, srt[-1] - srt[-2]


def detect_instance(score_map, masks, class_id, max_fragment_size=0):
    """the reference's dict; arrays with a leading dimension of 0 when every mask is empty"""
    score, cls, out = [], [], []
    for sc, mk, c in zip(score_map, masks, class_id):
        lab, n = cc_label(mk)
        for f in range(1, n + 1):
            seg = lab == f
            score.append(0 if seg.sum() < max_fragment_size else np.max(sc * seg))
            cls.append(c)
            out.append(seg)
    if not out:
        return {"score": np.zeros(0, np.float32), "mask": np.zeros((0,) + tuple(np.shape(masks)[1:]), bool),
                "class": np.zeros(0, np.int64)}
    return {"score": np.stack(score, 0), "mask": np.stack(out, 0), "class": np.stack(cls, 0)}


def make_ins_seg(cam, edge, dp, size, beta=10, exp_times=8, ins_seg_bg_thres=0.25):
    """every stage, float64 where the reference is float32 -> dict of the stages and the final dict"""
    cen = find_centroids(dp)
    inst, K = instance_map(cen, dp)
    h, w = inst.shape
    cams = resize_align_corners(cam, h, w)
    icam = cams[None] * (inst[None] == np.arange(K)[:, None, None])
    rw = propagate_to_edge(icam, edge, beta, exp_times)
    up, labels, gap = finish(rw, size, ins_seg_bg_thres)
    masks = labels[None] == np.arange(1, K + 1)[:, None, None]
    det = detect_instance(up, masks, np.zeros(K, np.int64), size[0] * size[1] * 0.01)
    det["cam"] = up
    return {"centroids": cen, "instance_map": inst, "K": K, "instance_cam": icam, "rw": rw, "rw_up": up, "labels": labels,
            "gap": gap, "detected": det}


# ------------------------------------------------------------------------------- reading tests/golden/g14_insseg.npz
def scenes(g):
    for i in range(int(g["n_scenes"])):
        s = {k[len(f"s{i}_"):]: g[k] for k in g.files if k.startswith(f"s{i}_")}
        s["det_mask"] = np.unpackbits(s["det_mask_bits"])[:int(np.prod(s["det_mask_shape"]))].reshape(s["det_mask_shape"]).astype(bool)
        s["size"] = tuple(int(v) for v in s["size"])
        yield i, s


def golden_paths(g):
    out, at = set(), 0
    for n in g["path_len"].astype(int):
        cells = [tuple(int(v) for v in c) for c in g["path_cells"][at:at + n]]
        at += n
        out.add((cells[0], frozenset(cells)))       # the reference lists the destination first
    return out
