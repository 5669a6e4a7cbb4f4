"""TRIS Stage-2 model on MI355X kernels -- drop-in for the reference's `model.model_stage2`
(/root/reference/model/model_stage2.py): `ConvBNRelu`, `Upsample`, `TRIS(args)` and `criterion`, the same 625 state-dict keys,
`.trainable_parameters()` and

    forward(x [B,3,H,W], word_id [B,T]) -> train: (seg_final_out1, seg_final_out2, seg_final_out3, seg_final_out4), each [B,1,H,W]
                                           eval : seg_final_out1

The maps are signed logits (no ReLU): `validate` evaluates them with ops.eval_post_signed (class attribute `signed_maps`).
Inside, activations are channels-last [B,h,w,C]: the RN50 trunk's taps c1..c4 feed PixelAttention (c2..c4) and the decoder, whose
3x3 convolutions carry the BatchNorm statistics in their epilogue (ops.conv3x3 stats=True) and whose BatchNorm + PReLU, upsample +
skip add, one-channel heads and loss are the kernels of csrc/seg.hip.
"""
import torch
from torch import nn

from .. import ops
from ..CLIP import clip
from ..CLIP.clip.model import BatchNorm2d, Conv2d
from .attn import PixelAttention


class PReLU(nn.Module):
    """nn.PReLU() -- ONE slope shared by all channels, initialised to 0.25 (the reference's default)"""

    def __init__(self, num_parameters=1, init=0.25):
        super().__init__()
        self.weight = nn.Parameter(torch.full((num_parameters,), float(init)))


class ConvBNRelu(nn.Module):
    """model_stage2.py:11-27: Conv2d(bias=False) -> BatchNorm2d -> PReLU.  Only the form Stage-2 builds (3x3, stride 1, padding 1,
    dilation 1, with the PReLU) is implemented; any other raises."""

    def __init__(self, in_planes, out_planes, kernel_size, stride=1, padding=0, dilation=1, G=32, use_relu=True):
        super().__init__()
        if (kernel_size, stride, padding, dilation, bool(use_relu)) != (3, 1, 1, 1, True):
            raise NotImplementedError(f"ConvBNRelu(kernel_size={kernel_size}, stride={stride}, padding={padding}, dilation={dilation}, "
                                      f"use_relu={use_relu}): Stage-2 builds only 3x3 / stride 1 / padding 1 with PReLU")
        self.use_relu = True
        self.conv = Conv2d(in_planes, out_planes, 3)
        self.bn = BatchNorm2d(out_planes)
        self.relu = PReLU()

    def forward_cl(self, x):
        """x channels-last [B,H,W,Cin] -> [B,H,W,Cout]"""
        tr = self.training
        y = ops.conv3x3(x, self.conv.weight, 1, stats=tr)
        if tr:
            self.bn._nbt_pending += 1
        bn = self.bn
        return ops.bn_prelu(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.relu.weight, tr, bn.momentum, bn.eps)

    def forward(self, x):
        """NCHW in / out, as the reference module"""
        return self.forward_cl(x.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)


def Upsample(x, size):
    """model_stage2.py:29-35: bilinear, align_corners=False, on an NCHW tensor"""
    return ops.resize_bilinear(x, size, False)


class _Head(nn.Sequential):
    """final_seg_k = Sequential(ConvBNRelu(C, C', 3, 1, 1), Conv2d(C', 1, 1, bias=False)) (model_stage2.py:75-86)"""

    def __init__(self, cin, cmid):
        super().__init__(ConvBNRelu(cin, cmid, kernel_size=3, stride=1, padding=1), Conv2d(cmid, 1, 1))

    def forward_cl(self, x, size):
        """channels-last x -> the logit map upsampled to the image size (H, W), [B,1,H,W]"""
        y = ops.head1x1(self[0].forward_cl(x), self[1].weight)          # [B,1,h,w]
        return ops.resize_bilinear(y, size, False)


class TRIS(nn.Module):
    signed_maps = True   # tris_amd.validate: the maps are signed logits (ops.eval_post_signed)

    def __init__(self, args=None):
        super().__init__()
        self.args = args
        self.clip = "clip" in args.bert_tokenizer
        if args.backbone not in ("clip-RN50", "clip-RN101"):
            raise ValueError(f"backbone {args.backbone!r} has no Stage-2 definition in the reference "
                             "(model_stage2.py:52-57 defines the channel widths of clip-RN50 / clip-RN101 only)")
        device = "cuda" if torch.cuda.is_available() else "cpu"
        clip_model, _ = clip.load(args.backbone.split("-")[-1], device=device, jit=False, txt_length=args.max_query_len)
        self.backbone = clip_model.float()
        # Parameters no Stage-2 step reaches (torch's AdamW skips them; they must stay bit-unchanged): the text projection (the
        # projected EOT feature `hidden` is unused, model_stage2.py:109), the attention pool (the trunk's pooled output is unused)
        # and logit_scale.  The flags are set on THIS model's CLIP instance only (Stage-1 trains text_projection).
        for p in [self.backbone.text_projection, self.backbone.logit_scale] + list(self.backbone.visual.attnpool.parameters()):
            p._tris_no_grad_path = True
        self.textdim = 512
        v_chans = [256, 512, 1024, 2048]
        l_chans = self.textdim
        self.attention2 = PixelAttention(visual_channel=v_chans[1], language_channel=l_chans)
        self.attention3 = PixelAttention(visual_channel=v_chans[2], language_channel=l_chans)
        self.attention4 = PixelAttention(visual_channel=v_chans[3], language_channel=l_chans)
        self.reduced_c1 = ConvBNRelu(v_chans[0], 64, kernel_size=3, stride=1, padding=1)
        self.reduced_c2 = ConvBNRelu(v_chans[1], 128, kernel_size=3, stride=1, padding=1)
        self.reduced_c3 = ConvBNRelu(v_chans[2], 256, kernel_size=3, stride=1, padding=1)
        self.reduced_c4 = ConvBNRelu(v_chans[3], 512, kernel_size=3, stride=1, padding=1)
        self.final_seg1 = _Head(32, 32)
        self.final_seg2 = _Head(64, 32)
        self.final_seg3 = _Head(128, 64)
        self.final_seg4 = _Head(256, 64)
        self.output4 = ConvBNRelu(512, 256, kernel_size=3, stride=1, padding=1)
        self.output3 = ConvBNRelu(256, 128, kernel_size=3, stride=1, padding=1)
        self.output2 = ConvBNRelu(128, 64, kernel_size=3, stride=1, padding=1)
        self.output1 = ConvBNRelu(64, 32, kernel_size=3, stride=1, padding=1)

    def trainable_parameters(self):
        """model_stage2.py:93-101: every `backbone.*` parameter except the two positional embeddings -> backbone group; the rest
        (the positional embeddings included) -> head group"""
        backbone, head = [], []
        for k, v in self.named_parameters():
            if k.startswith("backbone") and "positional_embedding" not in k:
                backbone.append(v)
            else:
                head.append(v)
        print("Backbone with decay={}, Head={}".format(len(backbone), len(head)))
        return backbone, head

    # -------------------------------------------------------------------------------------------------------- halves
    def encode_visual(self, x):
        """the image-only half: the trunk's taps c1..c4, channels-last fp32 (operand planes unpacked)"""
        return tuple(ops.unplanes(c) for c in self.backbone.visual.forward_cl(x, taps=True))

    def _words(self, word_id):
        """all T token features after ln_final [N,T,512] -- the text runs unpacked: PixelAttention attends over every token,
        the padding behind EOT included (model_stage2.py:109,114)"""
        return self.backbone.encode_text(word_id)[0]

    def _decode(self, taps, lan, size, train):
        c1, c2, c3, c4 = taps

        def fuse(att, c):
            b, h, w, C = c.shape
            flat = c.reshape(b, h * w, C)
            return ops.axpy(att.forward_cl(flat, lan), flat, 1.0).reshape(b, h, w, C)   # attention_k(c_k, lan) + c_k

        dem1 = self.reduced_c1.forward_cl(c1)
        dem2 = self.reduced_c2.forward_cl(fuse(self.attention2, c2))
        dem3 = self.reduced_c3.forward_cl(fuse(self.attention3, c3))
        dem4 = self.reduced_c4.forward_cl(fuse(self.attention4, c4))
        seg_out4, in3 = ops.upsample_nhwc(self.output4.forward_cl(dem4), dem3.shape[1:3], skip=dem3)
        seg_out3, in2 = ops.upsample_nhwc(self.output3.forward_cl(in3), dem2.shape[1:3], skip=dem2)
        seg_out2, in1 = ops.upsample_nhwc(self.output2.forward_cl(in2), dem1.shape[1:3], skip=dem1)
        seg_out1 = self.output1.forward_cl(in1)
        out1 = self.final_seg1.forward_cl(seg_out1, size)
        if not train:
            return out1
        out4 = self.final_seg4.forward_cl(seg_out4, size)
        out3 = self.final_seg3.forward_cl(seg_out3, size)
        out2 = self.final_seg2.forward_cl(seg_out2, size)
        return out1, out2, out3, out4

    @torch.no_grad()
    def forward_pairs(self, vis_state, word_id, owner, out_size):
        """Evaluation of S (image, sentence) pairs: vis_state = encode_visual of G images, word_id [S,T], owner[k] = the image of
        sentence k; out_size = H or (H, W).  -> seg_final_out1 of every pair [S,1,H,W], the reference's per-sentence call
        (validate.py:173-179) for each."""
        assert not self.training
        idx = torch.as_tensor(list(owner), device=word_id.device, dtype=torch.long)
        taps = tuple(c.index_select(0, idx) for c in vis_state)
        size = (int(out_size), int(out_size)) if isinstance(out_size, int) else tuple(int(v) for v in out_size)
        return self._decode(taps, self._words(word_id), size, False)

    def forward(self, x, word_id):
        if self.training:
            ops.h2_auto_step()
        with ops.h2_auto_lock():
            lan = self._words(word_id)
            return self._decode(self.encode_visual(x), lan, (int(x.shape[2]), int(x.shape[3])), self.training)   # img_size = x.shape[2:]


def criterion(seg_final_out1, target):
    """model_stage2.py:139-141: F.binary_cross_entropy_with_logits(out, target.float(), reduction='mean'), any target dtype (the
    training step forms the four heads' losses in one launch chain, ops.bce4)"""
    return ops.bce(seg_final_out1, target)
