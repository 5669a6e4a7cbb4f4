"""Test inputs and a torch restatement (fp32 or fp64, CPU) of IRNet's affinity / displacement training losses: the contract of
tris_amd.irn_loss (csrc/irnloss.hip).  tools/gen_golden_irn_loss.py records what the reference's own code gives on these inputs
(tests/golden/g16_irn_loss.npz); tests/test_irn_loss_host.py holds the restatement against that record.

The inputs make the path maximum unambiguous in any arithmetic: a near-tie would send a gradient to another pixel in fp32 than in
fp64.  The logits of an image are a permutation of h w equally spaced values in [-6, 6); the displacements are multiples of 1/8
plus 1/16, so that no |.| is taken at 0.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_SHAPES = [(2, 21, 23, 10), (2, 40, 52, 10), (2, 12, 14, 5)]      # (B, h, w, radius)
PLATEAU_SHAPE = (1, 21, 24, 10)
SEED = 7


def inputs(B, h, w, seed=SEED):
    """-> (edge_out float32 [B,1,h,w], dp_out float32 [B,2,h,w], label uint8 [B,h,w]) as numpy arrays"""
    rng = np.random.default_rng(seed)
    n = h * w
    edge = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.float64) * 12.0 / n - 6.0
    edge = edge.reshape(B, 1, h, w).astype(np.float32)
    dp = (rng.integers(-64, 65, size=(B, 2, h, w)) / 8.0 + 1.0 / 16.0).astype(np.float32)
    label = np.zeros((B, h, w), np.uint8)
    bh, bw = (h + 1) // 2, w // 3 + 3
    for b in range(B):
        oy, ox = int(rng.integers(0, max(h // 2, 1))), int(rng.integers(0, max(w // 2, 1)))
        label[b, oy:oy + bh, ox:ox + bw] = 1
        label[b, rng.integers(0, h, 12), rng.integers(0, w, 12)] = 255
    label[:, :, -2:] = 255
    return edge, dp, label


def plateau_inputs():
    """logits drawn from {-0.5, 0, 0.5}: every path has several equal maxima; dp zero"""
    B, h, w, _ = PLATEAU_SHAPE
    rng = np.random.default_rng(SEED + 1)
    edge = (rng.integers(-1, 2, size=(B, 1, h, w)) * 0.5).astype(np.float32)
    _, _, label = inputs(B, h, w, SEED + 1)
    return edge, np.zeros((B, 2, h, w), np.float32), label


def reference_paths(radius, scan_order=False):
    """[((dy, dx), [cells in the reference's path order])]: the cells of the direction's bounding box whose squared distance to
    the line is below 1, sorted (stable) by -(|cy| + |cx|) as IRNet/misc/indexing.py:48 does (scan_order: left unsorted, to show
    that the order decides where the gradient of a tie goes)"""
    dirs = [(0, dx) for dx in range(1, radius)]
    dirs += [(dy, dx) for dy in range(1, radius) for dx in range(1 - radius, radius) if dy * dy + dx * dx < radius * radius]
    out = []
    for dy, dx in dirs:
        cells = [(cy, cx) for cy in range(0, dy + 1) for cx in range(min(0, dx), max(0, dx) + 1)
                 if (dy * cx - dx * cy) ** 2 < dy * dy + dx * dx]
        if not scan_order:
            cells.sort(key=lambda c: -abs(c[0]) - abs(c[1]))
        out.append(((dy, dx), cells))
    return out


@functools.lru_cache(maxsize=None)
def _gather_tables(h, w, radius, scan_order, device):
    """-> (directions grouped by ascending path length, [flat cell indices [P, L, hs ws] per length]): what PathIndex keeps as
    search_dst and path_indices (indexing.py:53-88), built once per map size"""
    r = radius - 1
    hs, ws = h - r, w - 2 * r
    paths = reference_paths(radius, scan_order)
    lengths = sorted({len(c) for _, c in paths})
    order = [p for L in lengths for p in paths if len(p[1]) == L]
    full = torch.arange(h * w).view(h, w)
    gathers = [torch.stack([torch.stack([full[cy:cy + hs, r + cx:r + cx + ws].reshape(-1) for cy, cx in cells])
                            for _, cells in order if len(cells) == L]).to(device) for L in lengths]
    return order, gathers


def losses(edge_out, dp_out, label, radius, scan_order=False):
    """the contract, in the dtype of edge_out (torch, CPU, differentiable): -> (losses [4], counts int64 [3] = N_bg, N_fg, N_neg).
    The path maximum is F.max_pool2d over the cells in the reference's order, gathered with one index_select per path length as
    AffinityDisplacementLoss.to_affinity does, so that its backward picks the cell the reference's backward picks and a pixel's
    gradient is accumulated by few index_add passes (one slice-add per path cell loses a digit in fp32); the sums are single
    torch.sum calls over all pairs, as train_irn.py:57-63 has them."""
    B, _, h, w = edge_out.shape
    r = radius - 1
    hs, ws = h - r, w - 2 * r
    order, gathers = _gather_tables(h, w, radius, scan_order, str(edge_out.device))
    sig = torch.sigmoid(edge_out).view(B, -1)
    affs = []
    for idx in gathers:                                                                               # [P, L, hs ws]
        dist = torch.index_select(sig, -1, idx.view(-1)).view(B, idx.shape[0], idx.shape[1], hs * ws)
        affs.append(1 - F.max_pool2d(dist, (idx.shape[1], 1)).squeeze(2))
    aff = torch.cat(affs, 1)                                                                          # [B, D, hs ws]
    lab = label.to(torch.int64)
    a = lab[:, :hs, r:r + ws].reshape(B, 1, -1)
    b = torch.stack([lab[:, dy:dy + hs, r + dx:r + dx + ws].reshape(B, -1) for (dy, dx), _ in order], 1)
    valid = (a < 21) & (b < 21)
    bg = (valid & (a == b) & (a == 0)).to(edge_out.dtype)
    fg = (valid & (a == b) & (a > 0)).to(edge_out.dtype)
    ng = (valid & (a != b)).to(edge_out.dtype)
    pos = -torch.log(aff + 1e-5)
    neg = -torch.log(1. + 1e-5 - aff)
    src = dp_out[:, :, :hs, r:r + ws]
    pd = src.unsqueeze(2) - torch.stack([dp_out[:, :, dy:dy + hs, r + dx:r + dx + ws] for (dy, dx), _ in order], 2)
    pd = pd.reshape(B, 2, len(order), -1)                                                             # [B, 2, D, hs ws]
    tgt = torch.tensor([d for d, _ in order], dtype=dp_out.dtype, device=dp_out.device).t().reshape(1, 2, -1, 1)            # channel 0: dy, 1: dx
    n = [torch.sum(t) for t in (bg, fg, ng)]                     # (in the maps' dtype, as the reference; exact below 2^24)
    out = torch.stack([torch.sum(bg * pos) / (n[0] + 1e-5) / 2 + torch.sum(fg * pos) / (n[1] + 1e-5) / 2,
                       torch.sum(ng * neg) / (n[2] + 1e-5),
                       torch.sum((pd - tgt).abs() * fg.unsqueeze(1)) / (2 * n[1] + 1e-5),
                       torch.sum(pd.abs() * bg.unsqueeze(1)) / (2 * n[0] + 1e-5)])
    return out, torch.stack(n).detach().to(torch.int64)


def total(l):
    return (l[0] + l[1]) / 2 + (l[2] + l[3]) / 2


def restated(edge, dp, label, radius, dtype, weights=None, scan_order=False):
    """numpy inputs -> (losses, counts, d edge_out, d dp_out) as numpy in `dtype`; the gradients are those of total(losses), or
    of losses @ weights"""
    e = torch.from_numpy(edge).to(dtype).requires_grad_(True)
    d = torch.from_numpy(dp).to(dtype).requires_grad_(True)
    l, n = losses(e, d, torch.from_numpy(label), radius, scan_order)
    obj = total(l) if weights is None else (l * torch.tensor(weights, dtype=dtype)).sum()
    ge, gd = torch.autograd.grad(obj, (e, d), allow_unused=True)
    ge = torch.zeros_like(e) if ge is None else ge
    gd = torch.zeros_like(d) if gd is None else gd
    return l.detach().numpy(), n.numpy(), ge.numpy(), gd.numpy()


def rel_l2(a, b):
    """|a - b| / |b| in float64 (0 when both vanish)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))
