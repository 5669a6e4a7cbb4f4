"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference's Stage-2 model (model/model_stage2.py:11-141) over a flat state dict,
built on oracle.tris_oracle's encoders and PixelAttention.  Run it in fp64 to check the HIP path."""
import torch
import torch.nn.functional as F

from oracle import tris_oracle as O


def prelu_keys(sd):
    return sorted(k for k in sd if k.endswith(".relu.weight"))


def reset_slopes(sd, seed=5):
    """seed_fill sets every 1-D weight near 1, which hides the PReLU: put the slopes at 0.25 +- 0.05"""
    g = torch.Generator().manual_seed(seed)
    for k in prelu_keys(sd):
        sd[k].copy_(0.25 + 0.05 * (2 * torch.rand(sd[k].shape, generator=g) - 1))


def cbr(sd, p, x, train):
    """ConvBNRelu: 3x3 conv (bias=False) -> BatchNorm2d -> PReLU (:11-27)"""
    y = F.conv2d(x, sd[p + ".conv.weight"], padding=1)
    y = F.batch_norm(y, sd[p + ".bn.running_mean"], sd[p + ".bn.running_var"], sd[p + ".bn.weight"], sd[p + ".bn.bias"], train,
                     0.1, 1e-5)
    return F.prelu(y, sd[p + ".relu.weight"])


def up(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False)


def head(sd, p, x, size):
    return up(F.conv2d(cbr(sd, p + ".0", x, head.train), sd[p + ".1.weight"]), size)


def forward(sd, img, ids, train):
    """TRIS.forward (:105-137) -> four maps (train) / seg_final_out1 (eval)"""
    c1, c2, c3, c4 = O.encode_image_rn(sd, "backbone.", img, train)
    words, _ = O.encode_text(sd, "backbone.", ids)
    lan = words.permute(0, 2, 1)
    f2 = O.pixel_attention(sd, "attention2", c2, lan) + c2
    f3 = O.pixel_attention(sd, "attention3", c3, lan) + c3
    f4 = O.pixel_attention(sd, "attention4", c4, lan) + c4
    dem1 = cbr(sd, "reduced_c1", c1, train)
    dem2 = cbr(sd, "reduced_c2", f2, train)
    dem3 = cbr(sd, "reduced_c3", f3, train)
    dem4 = cbr(sd, "reduced_c4", f4, train)
    s4 = up(cbr(sd, "output4", dem4, train), dem3.shape[2:])
    s3 = up(cbr(sd, "output3", s4 + dem3, train), dem2.shape[2:])
    s2 = up(cbr(sd, "output2", s3 + dem2, train), dem1.shape[2:])
    s1 = cbr(sd, "output1", s2 + dem1, train)
    size = img.shape[2:]
    head.train = train
    o1 = head(sd, "final_seg1", s1, size)
    if not train:
        return o1
    return o1, head(sd, "final_seg2", s2, size), head(sd, "final_seg3", s3, size), head(sd, "final_seg4", s4, size)


def losses(outs, target):
    """criterion of each head (:139-141), loss = l1 + l2 + l3 + l4 (train_stage2.py:314-319)"""
    ls = [F.binary_cross_entropy_with_logits(o, target.to(o.dtype), reduction="mean") for o in outs]
    return [ls[0] + ls[1] + ls[2] + ls[3]] + ls


def groups(sd_param_names):
    """trainable_parameters (:93-101): names of the backbone / head groups"""
    bb = [k for k in sd_param_names if k.startswith("backbone") and "positional_embedding" not in k]
    hd = [k for k in sd_param_names if not (k.startswith("backbone") and "positional_embedding" not in k)]
    return bb, hd
