"""Plain-torch restatement of the IRNet edge / displacement network (inference), written from its description: a torchvision-layout
ResNet-50 with strides (2, 2, 2, 1) and frozen BatchNorm, five edge branches and seven displacement branches of 1x1 convolution +
GroupNorm (+ bilinear upsample, + crop) + ReLU, and EdgeDisplacement.forward's flip-average.  Runs in fp32 or fp64 on the CPU from
a state dict with the canonical names (tris_amd.irn_net).  Test infrastructure: the product never imports it."""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
LAYERS = (3, 4, 6, 3)
STRIDES = (1, 2, 2, 1)
EDGE_UP = (1, 1, 2, 4, 4)
EDGE_GROUPS = 4
DP_GROUPS = (8, 16, 16, 16, 16, 16, 16)


def normalize(img_u8):
    """uint8 [H,W,3] (or grey [H,W]) -> float32 [3,H,W]: (u8 / 255 - mean) / std in float64, stored as float32"""
    a = np.asarray(img_u8)
    if a.ndim == 2:
        a = np.stack([a, a, a], 2)
    out = np.empty(a.shape, np.float32)
    for c in range(3):
        out[..., c] = (a[..., c] / 255. - MEAN[c]) / STD[c]
    return torch.from_numpy(out.transpose(2, 0, 1).copy())


def batch_of(img_u8):
    """[img, flip_w(img)] as float32 [2,3,H,W]"""
    x = normalize(img_u8)
    return torch.stack([x, x.flip(-1)])


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], training=False, eps=1e-5)


def _bottleneck(x, sd, p, stride):
    out = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"]), sd, p + ".bn1"))
    out = F.relu(_bn(F.conv2d(out, sd[p + ".conv2.weight"], stride=stride, padding=1), sd, p + ".bn2"))
    out = _bn(F.conv2d(out, sd[p + ".conv3.weight"]), sd, p + ".bn3")
    if p + ".downsample.0.weight" in sd:
        x = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"], stride=stride), sd, p + ".downsample.1")
    return F.relu(out + x)


def trunk(x, sd):
    """-> [x1 .. x5]"""
    x = F.relu(_bn(F.conv2d(x, sd["resnet50.conv1.weight"], stride=2, padding=3), sd, "resnet50.bn1"))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    taps = [x]
    for i, (n, stride) in enumerate(zip(LAYERS, STRIDES)):
        for j in range(n):
            x = _bottleneck(x, sd, f"resnet50.layer{i + 1}.{j}", stride if j == 0 else 1)
        taps.append(x)
    return taps


def _branch(x, sd, p, groups, up=1, relu=True):
    y = F.group_norm(F.conv2d(x, sd[p + ".0.weight"]), groups, sd[p + ".1.weight"], sd[p + ".1.bias"], eps=1e-5)
    if up > 1:
        y = F.interpolate(y, scale_factor=up, mode="bilinear", align_corners=False)
    return F.relu(y) if relu else y


def forward(sd, x, dtype=torch.float32):
    """sd: canonical state dict, x [2,3,H,W] = [img, flip_w(img)] -> dict(taps, edge_out [2,1,h,w], dp_out [2,2,h,w], edge [1,h,w],
    dp [2,h,w])"""
    sd = {k: v.detach().to("cpu").to(dtype) for k, v in sd.items() if v.is_floating_point()}
    x = x.to(dtype)
    with torch.no_grad():
        t = trunk(x, sd)
        h, w = t[1].shape[2:]
        e = [_branch(t[i], sd, f"fc_edge{i + 1}", EDGE_GROUPS, EDGE_UP[i])[..., :h, :w] for i in range(5)]
        edge_out = F.conv2d(torch.cat(e, 1), sd["fc_edge6.weight"], sd["fc_edge6.bias"])
        dp1 = _branch(t[0], sd, "fc_dp1", DP_GROUPS[0])
        dp2 = _branch(t[1], sd, "fc_dp2", DP_GROUPS[1])
        dp3 = _branch(t[2], sd, "fc_dp3", DP_GROUPS[2])
        h3, w3 = dp3.shape[2:]
        dp4 = _branch(t[3], sd, "fc_dp4", DP_GROUPS[3], 2)[..., :h3, :w3]
        dp5 = _branch(t[4], sd, "fc_dp5", DP_GROUPS[4], 2)[..., :h3, :w3]
        up3 = _branch(torch.cat([dp3, dp4, dp5], 1), sd, "fc_dp6", DP_GROUPS[5], 2)[..., :dp2.shape[2], :dp2.shape[3]]
        a7 = _branch(torch.cat([dp1, dp2, up3], 1), sd, "fc_dp7", DP_GROUPS[6])
        dp_out = F.conv2d(a7, sd["fc_dp7.3.weight"]) - sd["mean_shift.running_mean"].view(1, 2, 1, 1)
        fh, fw = (x.shape[2] - 1) // 4 + 1, (x.shape[3] - 1) // 4 + 1
        edge_out, dp_out = edge_out[..., :fh, :fw], dp_out[..., :fh, :fw]
        edge = torch.sigmoid(edge_out[0] / 2 + edge_out[1].flip(-1) / 2)
    return {"taps": t, "edge_out": edge_out, "dp_out": dp_out, "edge": edge, "dp": dp_out[0]}


# ---- the recording (tools/gen_golden_irn.py) ---------------------------------------------------------------------------------
# (H, W, grey): 65 x 97 -> a 17 x 25 map (both odd: the x2 and x4 upsampled maps overhang) whose stride-8 map 9 x 13 is odd too;
# 72 x 50 grey -> 18 x 13, stride-8 9 x 7; 64 x 96 -> no crop bites
IMAGES = ((65, 97, False), (72, 50, True), (64, 96, False))
TAP_IMAGE = 0


def tap_stride(numel):
    """the fixed stride of the recorded sample of a tap (the five taps of one image whole would be 2.4 MB)"""
    return max(1, -(-numel // 16384)) | 1


def tap_sample(t):
    f = t.reshape(-1)
    return f[::tap_stride(f.numel())]


def images():
    from tris_amd.utils.synth import irn_image
    return [irn_image(H, W, seed=100 + i, grey=g) for i, (H, W, g) in enumerate(IMAGES)]


def filled_state_dict(seed, gain, module=None):
    """the seeded weights of the recording as a canonical state dict (float32, CPU)"""
    from tris_amd.irn_net import EdgeDisplacement
    from tris_amd.utils.synth import irn_fill
    m = EdgeDisplacement() if module is None else module
    return irn_fill(m.state_dict(), seed, gain)
