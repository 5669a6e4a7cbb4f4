"""The IRNet edge / displacement network on the MI355X, inference only (csrc/irnnet.hip + the dense-product paths of ops).

    net = EdgeDisplacement()
    net.load_state_dict(torch.load(weights))          # a file IRNet's train_irn.py saved, or one with canonical names only
    edge, dp = net.cuda()(img_u8)                      # [h,w], [2,h,w] with h = (H-1)//4 + 1: EdgeDisplacement.forward's outputs

The module is a holder of parameters and buffers under the reference's names (IRNet/net/resnet50_irn.py, IRNet/net/resnet50.py);
the computation is HIP kernels on channels-last activations: the ResNet-50 trunk's 1x1 and 3x3 products on the MFMA paths
(ops.linear, ops.conv3x3), frozen BatchNorm as tris_bn_apply_f32 with an invstd formed once at load time, and the stem, pooling,
GroupNorm / upsample / concatenation, narrow heads and flip-average of csrc/irnnet.hip.  Both flip rows go through the network as
one B = 2 batch.  There is no CPU path: without a GPU forward raises ops.NoGpuError.

The wiring of fc_edge1..6 and fc_dp1..7 is stated once, in the tables EDGE / DP / BUFFERS below: the module construction, the
forward of both branches (run_heads, which inference and training share) and the trainable-parameter order
(head_parameter_names) are read off them.  Training the two branches is tris_amd.irn_train, whose
backward walks the same tables; the CRF labels it trains on are tris_amd.crf.

In the h2 arithmetic the products read fp32 activations and split them in their own loops (operand planes are a training-step
construct: they are not used here).  The products take the cost model's tile choice (ops.autotune_off): image sizes change from
call to call, and nothing may be cached per shape.
"""
import re
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import ops

MEAN = (0.485, 0.456, 0.406)     # TorchvisionNormalize (IRNet/voc12/dataloader.py:68)
STD = (0.229, 0.224, 0.225)
LAYERS = (3, 4, 6, 3)
STRIDES = (1, 2, 2, 1)           # of layer1..4: resnet50(strides=[2, 2, 2, 1]); strides[0] is the stem's
BN_EPS = 1e-5
GN_EPS = 1e-5
# One GroupNorm branch (IRNet/net/resnet50_irn.py:29-86): relu(upsample(groupnorm(conv1x1(src)), x scale)), cropped, written into
# channels [off, off + cout) of the buffer dst.  src: a tap index (x1..x5 are 0..4) or the buffer a branch before it filled.
Branch = namedtuple("Branch", "name src cin cout groups scale dst off")
# The narrow 1x1 convolution that closes a group of branches: it reads the buffer src
Head = namedtuple("Head", "name src cin cout bias")
EDGE = (Branch("fc_edge1", 0, 64, 32, 4, 1, "cat_e", 0),
        Branch("fc_edge2", 1, 256, 32, 4, 1, "cat_e", 32),
        Branch("fc_edge3", 2, 512, 32, 4, 2, "cat_e", 64),
        Branch("fc_edge4", 3, 1024, 32, 4, 4, "cat_e", 96),
        Branch("fc_edge5", 4, 2048, 32, 4, 4, "cat_e", 128))
EDGE_HEAD = Head("fc_edge6", "cat_e", 160, 1, True)
DP = (Branch("fc_dp1", 0, 64, 64, 8, 1, "cat7", 0),
      Branch("fc_dp2", 1, 256, 128, 16, 1, "cat7", 64),
      Branch("fc_dp3", 2, 512, 256, 16, 1, "cat6", 0),
      Branch("fc_dp4", 3, 1024, 256, 16, 2, "cat6", 256),
      Branch("fc_dp5", 4, 2048, 256, 16, 2, "cat6", 512),
      Branch("fc_dp6", "cat6", 768, 256, 16, 2, "cat7", 192),
      Branch("fc_dp7", "cat7", 448, 256, 16, 1, "a7", 0))
DP_HEAD = Head("fc_dp7.3", "a7", 256, 2, False)
GROUPS = {"edge": (EDGE, EDGE_HEAD), "dp": (DP, DP_HEAD)}
# buffer -> (channels, the tap whose height and width it has)
BUFFERS = {"cat_e": (160, 1), "cat6": (768, 2), "cat7": (448, 1), "a7": (256, 1)}


# buffers of AffinityDisplacementLoss (IRNet/net/resnet50_irn.py:161-166) that a checkpoint saved by train_irn.py carries
TRAINING_ONLY = re.compile(r"path_indices\d+|disp_target")


def normalize_table():
    """float32 [3,256]: (v / 255 - mean) / std in float64, rounded once -- what TorchvisionNormalize stores for a uint8 v"""
    v = np.arange(256, dtype=np.float64)
    return torch.from_numpy(np.stack([((v / 255. - m) / s).astype(np.float32) for m, s in zip(MEAN, STD)]))


def branch_names(b):
    """the parameters of a Branch: its convolution weight, GroupNorm scale and GroupNorm bias"""
    return f"{b.name}.0.weight", f"{b.name}.1.weight", f"{b.name}.1.bias"


def head_parameter_names():
    """(edge names, dp names): the reference's trainable_parameters() (resnet50_irn.py:141-143), canonical names in its order"""
    return tuple([n for b in branches for n in branch_names(b)] + [f"{head.name}.weight"] + [f"{head.name}.bias"] * head.bias
                 for branches, head in GROUPS.values())


def run_heads(taps, prm, dp_bias=None, record=None, only=None):
    """Net.forward's two branches (IRNet/net/resnet50_irn.py:123-139) on the taps x1..x5 (channels-last): -> {"edge": [B,h,w,1],
    "dp": [B,h,w,2]}.  prm: canonical name -> tensor for every name of head_parameter_names().  dp_bias: what fc_dp7[3] adds --
    inference passes -mean_shift.running_mean, training nothing (MeanShift is the identity in train mode, :111-114).  record: a
    dict that receives the buffers of BUFFERS and, under "gn", {branch name: (GroupNorm input, statistics)}: what a backward
    needs.  only: "edge" | "dp" runs that group alone."""
    B, dev = taps[0].shape[0], taps[0].device
    bufs, gn, out = {}, {}, {}
    for key in GROUPS if only is None else (only,):
        branches, head = GROUPS[key]
        for b in branches:
            if b.dst not in bufs:
                C, tap = BUFFERS[b.dst]
                bufs[b.dst] = torch.empty(B, *taps[tap].shape[1:3], C, dtype=torch.float32, device=dev)
            dst = bufs[b.dst]
            conv, gamma, beta = (prm[n] for n in branch_names(b))
            t = ops.linear(taps[b.src] if isinstance(b.src, int) else bufs[b.src], conv)
            st = ops.group_norm_stats(t, b.groups, GN_EPS)
            gn[b.name] = (t, st)
            ops.gn_apply_up(t, st, gamma, beta, b.groups, b.scale, dst.shape[1:3], True, dst, b.off)
        bias = prm[f"{head.name}.bias"] if head.bias else dp_bias
        out[key] = ops.irn_head(bufs[head.src], prm[f"{head.name}.weight"].reshape(head.cout, head.cin), bias)
    if record is not None:
        record.update(bufs, gn=gn)
    return out


def feat_size(H, W):
    return (H - 1) // 4 + 1, (W - 1) // 4 + 1


def canonical_name(key):
    """the canonical name of a state-dict key of the reference's Net, which registers its modules several times (stage1..5,
    backbone, edge_layers, dp_layers, and the mean shift inside fc_dp7); canonical keys map to themselves"""
    m = re.match(r"backbone\.(\d+)\.(.*)", key)
    if m:
        key = f"stage{int(m.group(1)) + 1}.{m.group(2)}"
    m = re.match(r"edge_layers\.(\d+)\.(.*)", key)
    if m:
        key = f"fc_edge{int(m.group(1)) + 1}.{m.group(2)}"
    m = re.match(r"dp_layers\.(\d+)\.(.*)", key)
    if m:
        key = f"fc_dp{int(m.group(1)) + 1}.{m.group(2)}"
    m = re.match(r"stage1\.([01])\.(.*)", key)
    if m:
        return f"resnet50.{('conv1', 'bn1')[int(m.group(1))]}.{m.group(2)}"
    m = re.match(r"stage([2-5])\.0\.(.*)", key)
    if m:
        return f"resnet50.layer{int(m.group(1)) - 1}.{m.group(2)}"
    if key == "fc_dp7.4.running_mean":
        return "mean_shift.running_mean"
    return key


class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.stride = stride
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
        else:
            self.downsample = None


class _Trunk(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for i, (n, stride) in enumerate(zip(LAYERS, STRIDES)):
            planes = 64 << i
            blocks = [_Bottleneck(inplanes, planes, stride, True)]
            inplanes = planes * 4
            blocks += [_Bottleneck(inplanes, planes, 1, False) for _ in range(1, n)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))


class _MeanShift(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("running_mean", torch.zeros(2))


class EdgeDisplacement(nn.Module):
    """Parameters and buffers under the reference's canonical names: resnet50.*, fc_edge1..6.*, fc_dp1..7.*,
    mean_shift.running_mean.  forward(img_u8 [H,W,3]) -> (edge [h,w], dp [2,h,w]) float32 on the device."""

    def __init__(self):
        super().__init__()
        self.resnet50 = _Trunk()
        self.mean_shift = _MeanShift()
        for branches, head in GROUPS.values():
            for b in branches:
                setattr(self, b.name, nn.Sequential(nn.Conv2d(b.cin, b.cout, 1, bias=False), nn.GroupNorm(b.groups, b.cout)))
            conv = nn.Conv2d(head.cin, head.cout, 1, bias=head.bias)
            if head is EDGE_HEAD:
                self.fc_edge6 = conv
            else:
                self.fc_dp7.extend([nn.Identity(), conv])     # fc_dp7[3], behind the place of the reference's ReLU
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        self._prep = None
        self.calls = 0          # network passes so far (make_ins_seg reuses the last image's result: its test reads this)

    # ------------------------------------------------------------------------------------------------------------ loading
    def load_state_dict(self, state_dict, strict=True, **kw):
        """accepts the reference's state dict, where every tensor appears under several names, and one with canonical names only.
        The file train_irn.py saves is AffinityDisplacementLoss's: its training-only buffers (TRAINING_ONLY) are passed over, as the
        reference's own strict=False load does (IRNet/step_refer/make_ins_seg_labels.py:172); strict=False passes over any other
        unknown key too.
        Raises KeyError when a canonical tensor is missing or a key maps to no tensor of the network, ValueError when two
        aliases of one tensor disagree or a shape is wrong."""
        own = super().state_dict()
        canon, first = {}, {}
        for k, v in state_dict.items():
            if TRAINING_ONLY.fullmatch(k):
                continue
            c = canonical_name(k)
            if c not in own:
                if not strict:
                    continue
                raise KeyError(f"EdgeDisplacement.load_state_dict: unexpected key {k!r}")
            v = torch.as_tensor(v)
            if tuple(v.shape) != tuple(own[c].shape):
                raise ValueError(f"EdgeDisplacement.load_state_dict: {k!r} has shape {tuple(v.shape)}, expected {tuple(own[c].shape)}")
            if c in canon:
                if not torch.equal(canon[c].cpu(), v.cpu()):
                    raise ValueError(f"EdgeDisplacement.load_state_dict: {k!r} and {first[c]!r} name the same tensor but disagree")
            else:
                canon[c], first[c] = v, k
        missing = [k for k in own if k not in canon]
        if missing:
            raise KeyError(f"EdgeDisplacement.load_state_dict: missing {len(missing)} tensors, first {missing[:3]}")
        out = super().load_state_dict(canon, strict=True)
        self._prep = None
        return out

    # ----------------------------------------------------------------------------------------------- load-time preparation
    def _versions(self):
        return tuple(t._version for t in self.state_dict(keep_vars=True).values())

    def _prepare(self, dev):
        """derived constants, formed once per load: 1/sqrt(running_var + eps) of every frozen BatchNorm (float64, rounded once),
        the stem weight as [7,7,3,64], 3x3 weights in the kernel layout, the heads' parameters by name, the normalisation table"""
        if any(t.device != dev for t in self.state_dict(keep_vars=True).values()):
            raise ops.NoGpuError("EdgeDisplacement: move the module to the GPU first (.cuda()); there is no CPU fallback")
        ver = self._versions()
        if self._prep is not None and self._prep["ver"] == ver:
            return self._prep
        inv = {}
        for name, m in self.named_modules():
            if isinstance(m, nn.BatchNorm2d):
                inv[m] = (1.0 / torch.sqrt(m.running_var.double() + BN_EPS)).float()
            if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3):
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
        r = self.resnet50
        self._prep = {
            "ver": self._versions(), "inv": inv, "lut": normalize_table().to(dev),
            "stem_w": r.conv1.weight.detach().permute(2, 3, 1, 0).contiguous(),
            "heads": {n: self.get_parameter(n) for names in head_parameter_names() for n in names},
            "dp_b": (-self.mean_shift.running_mean.detach()).contiguous(),
        }
        return self._prep

    # ------------------------------------------------------------------------------------------------------------- pieces
    def _bn(self, x, bn, resid=None, relu=True):
        return ops.bn_frozen(x, bn.running_mean, self._prep["inv"][bn], bn.weight, bn.bias, resid, relu)

    def _stem(self, img):
        r, p = self.resnet50, self._prep
        y = ops.irn_stem(img, p["lut"], p["stem_w"], r.bn1.running_mean, p["inv"][r.bn1], r.bn1.weight, r.bn1.bias)
        return ops.maxpool3s2(y)

    def _block(self, x, blk):
        out = self._bn(ops.linear(x, blk.conv1.weight), blk.bn1)
        out = self._bn(ops.conv3x3(out, blk.conv2.weight, blk.stride), blk.bn2)
        out = ops.linear(out, blk.conv3.weight)
        resid = x
        if blk.downsample is not None:
            resid = x if blk.stride == 1 else ops.subsample2(x)     # the strided 1x1 reads pixel (2i, 2j)
            resid = self._bn(ops.linear(resid, blk.downsample[0].weight), blk.downsample[1], relu=False)
        return self._bn(out, blk.bn3, resid=resid, relu=True)

    def _trunk(self, x1):
        taps, x = [x1], x1
        for i in range(4):
            for blk in getattr(self.resnet50, f"layer{i + 1}"):
                x = self._block(x, blk)
            taps.append(x)
        return taps

    def heads(self, taps, only=None):
        """run_heads in eval mode: the mean shift is subtracted in fc_dp7[3]'s bias"""
        return run_heads(taps, self._prep["heads"], self._prep["dp_b"], only=only)

    # ------------------------------------------------------------------------------------------------------------ forward
    def _image(self, img):
        if not torch.cuda.is_available():
            raise ops.NoGpuError("tris_amd.irn_net runs on MI355X only (no GPU in this process); there is no CPU fallback")
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.array(img, order="C"))     # (a copy: arrays decoded by Pillow are read-only)
        if img.dtype != torch.uint8 or img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] != 3):
            raise ValueError(f"EdgeDisplacement.forward takes a uint8 image [H,W,3], got {img.dtype} {tuple(img.shape)}")
        dev = self.fc_edge6.weight.device
        if dev.type != "cuda":
            raise ops.NoGpuError("EdgeDisplacement: move the module to the GPU first (.cuda()); there is no CPU fallback")
        img = img.to(dev)
        if img.dim() == 2:           # a grey image: three equal channels (IRNet/voc12/dataloader.py:328-330)
            img = img[:, :, None].expand(-1, -1, 3)
        return img.contiguous()

    @torch.no_grad()
    def forward_raw(self, img, taps=False):
        """-> {'edge_out' [2,h,w], 'dp_out' [2,h,w,2] (channels-last), 'edge' [h,w], 'dp' [2,h,w]} (+ 'taps': x1..x5 channels-last):
        the network's outputs for [img, flip_w(img)] before and after EdgeDisplacement.forward's flip-average"""
        img = self._image(img)
        self._prepare(img.device)
        self.calls += 1
        with ops.autotune_off():
            if ops.h2_on() and not ops.h2_step_open():
                ops.h2_begin_step(explicit=False)     # a fresh amax pool: the pass never straddles two
            t = self._trunk(self._stem(img))
            y = self.heads(t)
            edge_out, dp_out = y["edge"][..., 0], y["dp"]
            edge, dp = ops.irn_net_finish(edge_out, dp_out)
        out = {"edge_out": edge_out, "dp_out": dp_out, "edge": edge, "dp": dp}
        if taps:
            out["taps"] = t
        return out

    def forward(self, img):
        out = self.forward_raw(img)
        return out["edge"], out["dp"]
