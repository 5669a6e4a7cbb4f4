"""IRNet's affinity / displacement training losses on the MI355X (csrc/irnloss.hip): the loss head of the reference's
IRNet/step_refer/train_irn.py on AffinityDisplacementLoss (IRNet/net/resnet50_irn.py:168-222).

    from tris_amd import irn_loss
    losses, counts = irn_loss.affinity_displacement_losses(edge_out, dp_out, irn_loss.reduce_label(label_u8), radius=10)
    irn_loss.total_loss(losses).backward()            # fills the gradients of edge_out and dp_out

edge_out [B,1,h,w] (logits) and dp_out [B,2,h,w] are what the network's two heads return in train mode (MeanShift is the identity
there); label is the uint8 class map at the maps' size, from which the kernel derives the pair labels the reference's
GetAffinityLabelFromIndices builds on the host (IRNet/voc12/dataloader.py:83-109).  Nothing per pair is ever in memory
("IRNet training losses").  The backward of the heads and the optimiser are tris_amd.irn_train.
There is no CPU path: CPU tensors raise ops.NoGpuError.
"""
import numpy as np
import torch

from . import irn, ops


def affinity_displacement_losses(edge_out, dp_out, label, radius=10):
    """-> (losses float32 [4] = (pos_aff_loss, neg_aff_loss, dp_fg_loss, dp_bg_loss) of train_irn.py:57-63, counts int64 [3] =
    (N_bg, N_fg, N_neg), the pair counts over the batch); differentiable in edge_out and dp_out.  An empty class gives loss 0."""
    for t in (edge_out, dp_out, label):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"affinity_displacement_losses takes tensors, got {type(t).__name__}")
    ops.irn_loss_check(edge_out, dp_out, label, radius)
    if not (edge_out.is_cuda and dp_out.is_cuda and label.is_cuda):
        raise ops.NoGpuError("tris_amd.irn_loss runs on MI355X only (got a CPU tensor); there is no CPU fallback")
    return ops.irn_aff_losses(edge_out, dp_out, label, *irn.device_tables(edge_out.device, int(radius)), radius=int(radius))


def total_loss(losses):
    """train_irn.py:68: (pos_aff_loss + neg_aff_loss) / 2 + (dp_fg_loss + dp_bg_loss) / 2"""
    return (losses[0] + losses[1]) / 2 + (losses[2] + losses[3]) / 2


def reduce_label(label_u8):
    """the reference's imutils.pil_rescale(label, 0.25, 0) (IRNet/voc12/dataloader.py:281): Pillow NEAREST to
    (round(H / 4), round(W / 4)), halves to even as np.round; uint8 [H,W] -> [h,w] or [B,H,W] -> [B,h,w], bit for bit"""
    if not isinstance(label_u8, torch.Tensor) or label_u8.dim() not in (2, 3) or label_u8.dtype != torch.uint8:
        what = f"{tuple(label_u8.shape)} {label_u8.dtype}" if isinstance(label_u8, torch.Tensor) else type(label_u8).__name__
        raise ValueError(f"reduce_label takes a uint8 [H,W] or [B,H,W] tensor, got {what}")
    if not label_u8.is_cuda:
        raise ops.NoGpuError("tris_amd.irn_loss runs on MI355X only (got a CPU tensor); there is no CPU fallback")
    H, W = label_u8.shape[-2:]
    h, w = int(np.round(H * 0.25)), int(np.round(W * 0.25))
    if h < 1 or w < 1:
        raise ValueError(f"reduce_label: a {tuple(label_u8.shape)} label reduces to nothing")
    if label_u8.dim() == 2:
        return ops.resize_nearest_u8(label_u8, h, w)
    # the batch rides in the op's channel dimension: [B,H,W] -> [H,W,B] -> [h,w,B] -> [B,h,w]
    return ops.resize_nearest_u8(label_u8.permute(1, 2, 0).contiguous(), h, w).permute(2, 0, 1).contiguous()
