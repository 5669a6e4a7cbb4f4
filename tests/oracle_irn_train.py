"""Test inputs and a plain-torch restatement (fp32 or fp64, CPU) of one training iteration of IRNet's edge / displacement heads: the
contract of tris_amd.irn_train (csrc/irntrain.hip, tris_amd.optim.PolySGD).  It extends tests/oracle_irn.py (the frozen trunk) and
tests/oracle_irn_loss.py (the losses).  tools/gen_golden_irn_train.py records what the reference's own AffinityDisplacementLoss and
PolyOptimizer give on these inputs (tests/golden/g17_irn_train.npz); tests/test_irn_train_host.py holds the restatement against that
record.

Train-mode semantics restated: every tap is detached, the backbone is in eval mode, MeanShift is the identity, no flip-average.
The ReLU masks can be IMPOSED from outside (masks=...): a pre-activation within rounding of zero has another sign in another
arithmetic, which moves a gradient by O(1) of that element's share -- a property of the input, not of the code under test -- so the
GPU's gradients are compared against fp64 gradients taken under the GPU's own masks, and the masks are compared separately.
"""
import numpy as np
import torch
import torch.nn.functional as F

import oracle_irn as O
import oracle_irn_loss as L

# (B, H, W, loss radius): 65 x 97 -> maps 17 x 25, stride-8 map 9 x 13: every x2 / x4 upsample overhangs and is cropped;
# 72 x 50 -> 18 x 13, stride-8 9 x 7 (13 < 21 columns: radius 5); 64 x 96 -> 16 x 24, no crop bites
SHAPES = ((2, 65, 97, 10), (3, 72, 50, 5), (2, 64, 96, 10))
STEP_SHAPE = 0                  # the shape of the recorded three-step run
LR, WEIGHT_DECAY, MAX_STEP, N_STEPS = 0.1, 1e-4, 5, 3
# GroupNorm branches: (name, tap or None, groups, upsample factor)
EDGE = (("fc_edge1", 0, 4, 1), ("fc_edge2", 1, 4, 1), ("fc_edge3", 2, 4, 2), ("fc_edge4", 3, 4, 4), ("fc_edge5", 4, 4, 4))
DP = (("fc_dp1", 0, 8, 1), ("fc_dp2", 1, 16, 1), ("fc_dp3", 2, 16, 1), ("fc_dp4", 3, 16, 2), ("fc_dp5", 4, 16, 2))
BRANCHES = tuple(n for n, *_ in EDGE) + tuple(n for n, *_ in DP) + ("fc_dp6", "fc_dp7")
SAMPLE = 3072                   # elements of a recorded parameter-sized tensor at most


def head_names():
    """(edge names, dp names) in the order of the reference's trainable_parameters()"""
    edge = [f"{n}.{s}" for n, *_ in EDGE for s in ("0.weight", "1.weight", "1.bias")] + ["fc_edge6.weight", "fc_edge6.bias"]
    dp = [f"{n}.{s}" for n in [n for n, *_ in DP] + ["fc_dp6"] for s in ("0.weight", "1.weight", "1.bias")]
    dp += ["fc_dp7.0.weight", "fc_dp7.1.weight", "fc_dp7.1.bias", "fc_dp7.3.weight"]
    return edge, dp


def sample(t):
    """the fixed strided sample under which a parameter-sized tensor is recorded"""
    f = t.reshape(-1)
    return f[::max(1, -(-f.numel() // SAMPLE)) | 1]


def map_size(H, W):
    return (H - 1) // 4 + 1, (W - 1) // 4 + 1


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def images(i, seed):
    """float32 [B,3,H,W]: normalised images as the training loader delivers them; the last one carries the random crop's padding,
    exact zeros written AFTER the normalisation, along its bottom and right edges"""
    from tris_amd.utils.synth import irn_image
    B, H, W, _ = SHAPES[i]
    x = torch.stack([O.normalize(irn_image(H, W, seed=1000 * seed + 10 * i + b)) for b in range(B)])
    x[-1, :, H - 9:, :] = 0.0
    x[-1, :, :, W - 6:] = 0.0
    return x


def labels(i, seed):
    """uint8 [B,h,w] at the maps' size with values from {0, 1, 2, 255}"""
    B, H, W, _ = SHAPES[i]
    h, w = map_size(H, W)
    rng = np.random.default_rng(77 * seed + i)
    lab = np.zeros((B, h, w), np.uint8)
    for b in range(B):
        y0, x0 = int(rng.integers(0, h // 3)), int(rng.integers(0, w // 3))
        lab[b, y0:y0 + h // 2, x0:x0 + w // 2] = 1
        y1, x1 = int(rng.integers(h // 3, h // 2)), int(rng.integers(w // 3, w // 2))
        lab[b, y1:y1 + h // 3, x1:x1 + w // 3] = 2
        lab[b, rng.integers(0, h, 6), rng.integers(0, w, 6)] = 255
    return torch.from_numpy(lab)


def cotangents(i, seed):
    """(Ge [B,1,h,w], Gd [B,2,h,w]) float32: the linear functional sum(Ge edge_out) + sum(Gd dp_out)"""
    B, H, W, _ = SHAPES[i]
    h, w = map_size(H, W)
    g = torch.Generator().manual_seed(500 + 31 * seed + i)
    return torch.randn(B, 1, h, w, generator=g), torch.randn(B, 2, h, w, generator=g)


# ---- the heads -----------------------------------------------------------------------------------------------------------------
def _branch(x, sd, p, groups, up, size, masks, pre):
    y = F.group_norm(F.conv2d(x, sd[p + ".0.weight"]), groups, sd[p + ".1.weight"], sd[p + ".1.bias"], eps=1e-5)
    if up > 1:
        y = F.interpolate(y, scale_factor=up, mode="bilinear", align_corners=False)
    y = y[..., :size[0], :size[1]]
    pre[p] = y
    return F.relu(y) if masks is None else y * masks[p].to(y.dtype)


def heads(sd, taps, masks=None):
    """sd: head tensors by canonical name (leaves that may require grad), taps x1..x5 [B,C,H,W] in the same dtype ->
    (edge_out [B,1,h,w], dp_out [B,2,h,w], pre: {branch name: pre-activation of its ReLU})"""
    pre = {}
    hw, hw3 = taps[1].shape[2:], taps[2].shape[2:]
    e = [_branch(taps[t], sd, n, g, up, hw, masks, pre) for n, t, g, up in EDGE]
    edge_out = F.conv2d(torch.cat(e, 1), sd["fc_edge6.weight"], sd["fc_edge6.bias"])
    d = [_branch(taps[t], sd, n, g, up, hw if t < 2 else hw3, masks, pre) for n, t, g, up in DP]
    up3 = _branch(torch.cat(d[2:], 1), sd, "fc_dp6", 16, 2, hw, masks, pre)
    a7 = _branch(torch.cat([d[0], d[1], up3], 1), sd, "fc_dp7", 16, 1, hw, masks, pre)
    return edge_out, F.conv2d(a7, sd["fc_dp7.3.weight"]), pre


def frozen_taps(sd, x, dtype):
    """the trunk's taps on a float batch [B,3,H,W], detached"""
    full = {k: v.detach().to("cpu").to(dtype) for k, v in sd.items() if v.is_floating_point()}
    with torch.no_grad():
        return [t.detach() for t in O.trunk(x.to(dtype), full)]


def head_leaves(sd, dtype):
    return {k: sd[k].detach().to("cpu").to(dtype).clone().requires_grad_(True) for names in head_names() for k in names}


def linear_functional(sd, x, Ge, Gd, dtype, masks=None, taps=None):
    """-> dict(edge_out, dp_out, grads {name: gradient of sum(Ge edge_out) + sum(Gd dp_out)}, pre, taps), all in `dtype`"""
    taps = frozen_taps(sd, x, dtype) if taps is None else taps
    p = head_leaves(sd, dtype)
    edge_out, dp_out, pre = heads(p, taps, masks)
    obj = (Ge.to(dtype) * edge_out).sum() + (Gd.to(dtype) * dp_out).sum()
    grads = dict(zip(p, torch.autograd.grad(obj, list(p.values()))))
    return {"edge_out": edge_out.detach(), "dp_out": dp_out.detach(), "grads": grads, "pre": {k: v.detach() for k, v in pre.items()},
            "taps": taps}


def own_masks(pre):
    return {k: v > 0 for k, v in pre.items()}


def masks_from_buffers(keep):
    """the ReLU masks of a GPU forward, from the buffers IrnTrainer.heads leaves in `keep` (channels-last) -> {branch: bool [B,C,h,w]}"""
    cut = lambda t, a, b: (t[..., a:b] > 0).permute(0, 3, 1, 2).cpu()
    m = {f"fc_edge{i + 1}": cut(keep["cat_e"], 32 * i, 32 * i + 32) for i in range(5)}
    m.update(fc_dp1=cut(keep["cat7"], 0, 64), fc_dp2=cut(keep["cat7"], 64, 192), fc_dp6=cut(keep["cat7"], 192, 448),
             fc_dp3=cut(keep["cat6"], 0, 256), fc_dp4=cut(keep["cat6"], 256, 512), fc_dp5=cut(keep["cat6"], 512, 768),
             fc_dp7=cut(keep["a7"], 0, 256))
    return m


def mask_disagreement(masks, pre64):
    """-> (fraction of elements whose mask differs from the sign of the fp64 pre-activation, the largest |pre| / rms among them)"""
    bad, total, worst = 0, 0, 0.0
    for k, p in pre64.items():
        diff = masks[k] != (p > 0)
        total += p.numel()
        bad += int(diff.sum())
        if bool(diff.any()):
            worst = max(worst, float(p[diff].abs().max() / p.pow(2).mean().sqrt()))
    return bad / total, worst


# ---- the optimiser and the loop ----------------------------------------------------------------------------------------------------
def poly_lr(initial, step, max_step, power=0.9):
    """the learning rates PolyOptimizer.step sets before update number `step` (0-based), in Python floats; None: left as they are"""
    if step < max_step:
        return [lr0 * (1 - step / max_step) ** power for lr0 in initial]
    return None


def sgd_step(params, grads, bufs, lr, momentum, weight_decay):
    """torch.optim.SGD's update on lists of tensors, in place; bufs: list holding None before the first step"""
    with torch.no_grad():
        for i, (p, g) in enumerate(zip(params, grads)):
            g = g + weight_decay * p
            bufs[i] = g.clone() if bufs[i] is None else bufs[i] * momentum + g
            p -= lr * bufs[i]


def train_steps(sd, x, label, radius, dtype, n=N_STEPS, lr=LR, weight_decay=WEIGHT_DECAY, max_step=MAX_STEP):
    """n iterations of the reference's loop restated -> (losses of step 0 [4], {name: parameter after n steps}, {name: before})"""
    taps = frozen_taps(sd, x, dtype)                 # the trunk is frozen: the taps do not change from step to step
    p = head_leaves(sd, dtype)
    before = {k: v.detach().clone() for k, v in p.items()}
    edge, dp = head_names()
    groups = [([p[k] for k in edge], 1 * lr), ([p[k] for k in dp], 10 * lr)]
    bufs = [[None] * len(g) for g, _ in groups]
    cur = [g_lr for _, g_lr in groups]
    first = None
    for step in range(n):
        edge_out, dp_out, _ = heads(p, taps)
        losses, _ = L.losses(edge_out, dp_out, label, radius)
        if first is None:
            first = losses.detach().clone()
        grads = dict(zip(p, torch.autograd.grad(L.total(losses), list(p.values()))))
        cur = poly_lr([g_lr for _, g_lr in groups], step, max_step) or cur
        for (params, _), b, lr_now, names in zip(groups, bufs, cur, (edge, dp)):
            # momentum = the weight-decay value: the reference passes it into torch.optim.SGD's momentum slot
            sgd_step(params, [grads[k] for k in names], b, lr_now, weight_decay, weight_decay)
    return first, {k: v.detach() for k, v in p.items()}, before


def rel_l2(a, b):
    return L.rel_l2(a, b)
