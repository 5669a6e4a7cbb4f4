"""Instance-mask synthesis: the post-network half of IRNet's make_ins_seg_labels on the MI355X (csrc/insseg.hip).

The functions carry the reference's names (IRNet/step_refer/make_ins_seg_labels.py, IRNet/misc/indexing.py) so that its callers
can switch by importing this module:

    from tris_amd import irn
    rw = irn.propagate_to_edge(instance_cam, edge, beta=10, exp_times=8, radius=5)

(response map, edge map, displacement field) come in as arrays; the edge / displacement network that produces the last two is
tris_amd.irn_net (inference; of its training only the losses are on this stack, tris_amd.irn_loss: INTEGRATION.md, "Stage 2").  numpy inputs are moved to the GPU and numpy comes back; CUDA tensors stay tensors, except
that detect_instance and make_ins_seg always return the reference's dict of numpy arrays.  There is
no CPU path: without a GPU every function raises ops.NoGpuError.

The transition matrix of indexing.py:112-139 (N x N, N = h w) is never formed: x T^(2^t) is evaluated as 2^t products v T with the
68 + 1 non-zeros per column taken from the 34-direction weight planes ("Instance-mask synthesis").
"""
import math

import numpy as np
import torch

from . import ops

RADIUS = 5


# ---------------------------------------------------------------------------------------------- search directions and paths
def search_dirs(radius=RADIUS):
    """the (dy, dx) search directions of PathIndex: dy = 0 with 0 < dx < r, then dy > 0 with dy^2 + dx^2 < r^2 (34 for r = 5)"""
    dirs = [(0, dx) for dx in range(1, radius)]
    dirs += [(dy, dx) for dy in range(1, radius) for dx in range(1 - radius, radius) if dy * dy + dx * dx < radius * radius]
    return dirs


def search_paths(radius=RADIUS):
    """[(direction, [path cells])]: the cells (y, x) of the direction's bounding box whose squared distance to the line through
    the origin and the direction is below 1, both ends included; the affinity of a pixel pair is 1 - the largest edge on them"""
    out = []
    for dy, dx in search_dirs(radius):
        len_sq = dy * dy + dx * dx
        cells = []
        for y in range(0, dy + 1):
            for x in range(min(0, dx), max(0, dx) + 1):
                cross = dy * x - dx * y
                if cross * cross < len_sq:        # (cross^2 / len_sq < 1, in integers)
                    cells.append((y, x))
        out.append(((dy, dx), cells))
    return out


_TABLES = {}


def device_tables(device, radius=RADIUS):
    """(dirs int32 [D,2], path_off int32 [D+1], path_cells int32 [C,2]) on `device`, built once"""
    key = (str(device), radius)
    t = _TABLES.get(key)
    if t is None:
        paths = search_paths(radius)
        dirs = np.asarray([d for d, _ in paths], np.int32)
        off = np.cumsum([0] + [len(c) for _, c in paths]).astype(np.int32)
        cells = np.asarray([c for _, cs in paths for c in cs], np.int32)
        t = _TABLES[key] = tuple(torch.from_numpy(a).to(device) for a in (dirs, off, cells))
    return t


# --------------------------------------------------------------------------------------------------------------- plumbing
def _dev(a, dtype):
    """-> (contiguous CUDA tensor of dtype, whether the caller passed numpy)"""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ops.NoGpuError("tris_amd.irn runs on MI355X only (got a CPU tensor); there is no CPU fallback")
        return a.to(dtype).contiguous(), False
    if not torch.cuda.is_available():
        raise ops.NoGpuError("tris_amd.irn runs on MI355X only (no GPU in this process); there is no CPU fallback")
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype), True


def _back(t, as_numpy):
    return t.cpu().numpy() if as_numpy else t


# ------------------------------------------------------------------------------------------------- the reference's functions
def find_centroids_with_refinement(displacement, iterations=300):
    """displacement float32 [2,h,w] -> int32 [2,h,w] centroids (y, x); bit-identical to the reference"""
    dp, as_np = _dev(displacement, torch.float32)
    return _back(ops.irn_centroids(dp, iterations), as_np)


def _instance_map(centroids, dp, thres=2.5):
    """-> (instance map int32 [h,w] on device, K)"""
    lab, cnt = ops.cc_label(ops.irn_weak_mask(dp, thres))
    inst, k = ops.irn_cluster(centroids, lab, int(cnt.item()))
    return inst, int(k.item())


def cluster_centroids(centroids, displacement, thres=2.5):
    """-> one-hot instance map bool [K,h,w]: pixels grouped by the weak-displacement region their centroid falls in"""
    dp, as_np = _dev(displacement, torch.float32)
    cen, _ = _dev(centroids, torch.int32)
    inst, K = _instance_map(cen, dp, thres)
    return _back(ops.irn_label_masks(inst, K, base=0).bool(), as_np)


def propagate_to_edge(x, edge, radius=5, beta=10, exp_times=8):
    """x [K,1,h,w] (any shape ending in h,w), edge [h,w] -> rw [K,1,h,w] = x (1 - edge) T^(2^exp_times)"""
    if radius != RADIUS:
        raise NotImplementedError(f"propagate_to_edge: radius {radius} (the kernels carry the radius-5 tables)")
    xt, as_np = _dev(x, torch.float32)
    et, _ = _dev(edge, torch.float32)
    h, w = xt.shape[-2:]
    et = et.reshape(h, w)
    dirs, off, cells = device_tables(xt.device, radius)
    Wt, colsum = ops.irn_affinity(et, dirs, off, cells, beta)
    rw = ops.irn_walk(xt.reshape(-1, h, w), et, Wt, colsum, dirs, 2 ** int(exp_times))
    return _back(rw.reshape(-1, 1, h, w), as_np)


def _fragments(rw_up, labels, K, class_id, max_fragment_size):
    """detect_instance on device tensors: rw_up [K,H,W], labels int32 [H,W] in 0..K"""
    return _detect(rw_up, ops.irn_label_masks(labels, K), class_id, max_fragment_size)


def _detect(rw_up, masks_u8, class_id, max_fragment_size):
    K, H, W = masks_u8.shape
    fl, counts = ops.cc_label(masks_u8)
    counts = counts.cpu().tolist()
    score, area, fm = ops.irn_fragments(fl, counts, rw_up, math.ceil(max_fragment_size))
    score, area = score.cpu().numpy(), area.cpu().numpy()
    small = area < max_fragment_size
    # np.stack over the reference's list of `0` and np.float32 entries: float32, float64 when mixed, int64 when all are 0
    if len(score) and small.all():
        score = np.zeros(len(score), np.int64)
    elif small.any():
        score = score.astype(np.float64)
    cls = np.repeat(np.asarray(class_id)[:K], counts) if len(counts) else np.zeros(0, np.int64)
    return {"score": score, "mask": fm.cpu().numpy().view(bool), "class": cls}


def detect_instance(score_map, mask, class_id, max_fragment_size=0):
    """score_map [K,H,W], mask bool [K,H,W], class_id [K] -> {'score' [F], 'mask' bool [F,H,W], 'class' [F]}: the 4-connected
    fragments of every row's mask in (row, raster) order, scored max(score * fragment), 0 below max_fragment_size pixels.
    Where the reference fails in np.stack([]) on all-empty masks, the arrays here have a leading dimension of 0."""
    sm, _ = _dev(score_map, torch.float32)
    mk, _ = _dev(mask, torch.uint8)
    return _detect(sm, mk, class_id, max_fragment_size)


def make_ins_seg(cam, edge, dp, size, beta=10, exp_times=8, ins_seg_bg_thres=0.25):
    """_work's body after the network (make_ins_seg_labels.py:138-162): cam [Hc,Wc] response map, edge [h,w], dp [2,h,w],
    size (H, W) with h = (H-1)//4 + 1 -> {'score', 'mask', 'class', 'cam'}"""
    camt, _ = _dev(cam, torch.float32)
    et, _ = _dev(edge, torch.float32)
    dpt, _ = _dev(dp, torch.float32)
    H, W = int(size[0]), int(size[1])
    h, w = et.shape
    cen = ops.irn_centroids(dpt)
    inst, K = _instance_map(cen, dpt)
    cams = ops.resize_bilinear(camt[None, None], (h, w), True)[0, 0]
    rw = propagate_to_edge(ops.irn_instance_cam(cams, inst, K), et, beta=beta, exp_times=exp_times)
    rw_up, labels = ops.irn_finish(rw[:, 0], (H, W), ins_seg_bg_thres)
    out = _fragments(rw_up, labels, K, np.zeros(K, np.int64), H * W * 0.01)
    out["cam"] = rw_up.cpu().numpy()
    return out
