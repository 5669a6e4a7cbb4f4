"""Records tests/golden/g16_irn_loss.npz from the REAL reference code, on the CPU, in fp32: IRNet's affinity / displacement
training losses on the inputs of tests/oracle_irn_loss.py.  Build-machine tool: the reference tree is not on the GPU machines,
and nothing that runs there reads it.

    python tools/gen_golden_irn_loss.py

What runs is the reference's: misc.indexing.PathIndex; AffinityDisplacementLoss.to_affinity / to_pair_displacement /
to_displacement_loss (IRNet/net/resnet50_irn.py:168-202), called as plain functions on a stand-in object that carries path_index,
n_path_lengths, _buffers and disp_target as AffinityDisplacementLoss.__init__ sets them (:158-166); the loss expressions of its
forward (:211-220); voc12.dataloader.GetAffinityLabelFromIndices (:83-109) for the pair labels; the loss lines of
step_refer/train_irn.py:57-68 are the body of a training loop and are written out here (masked_mean).  The reference's Net is never
constructed (its constructor asks model_zoo.load_url for weights); the packages the reference imports and this stack lacks are
stubbed as in tools/gen_golden_irn.py.

Recorded per shape (B, h, w, radius) of oracle_irn_loss.GOLDEN_SHAPES: the four losses, the three pair counts, the gradients of
the total loss in edge_out and dp_out; for the plateau case (equal maxima on every path) the gradient of (l0 + l1) / 2.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "g16_irn_loss.npz")


def reference_modules():
    from oracle.ref_shim import REF_ROOT

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules.setdefault(name, m)
        return sys.modules[name]

    for name in ("imageio", "cv2", "skimage", "skimage.measure", "pydensecrf", "pydensecrf.densecrf", "pydensecrf.utils"):
        stub(name)
    sys.modules["pydensecrf.utils"].unary_from_labels = None     # (misc/imutils.py imports the name; the CRF is never run)
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REF_ROOT, "IRNet"))
    import net.resnet50 as r50                      # noqa: E402  (the reference's)
    r50.model_zoo.load_url = lambda *a, **k: {}     # never download (and Net is never constructed here)
    torch.utils.model_zoo.load_url = r50.model_zoo.load_url
    import net.resnet50_irn as irn                  # noqa: E402
    from misc import indexing                       # noqa: E402
    import voc12.dataloader as dataloader           # noqa: E402
    return irn.AffinityDisplacementLoss, indexing.PathIndex, dataloader.GetAffinityLabelFromIndices


class StandIn:
    """what AffinityDisplacementLoss.__init__ sets (resnet50_irn.py:158-166), without the network"""

    def __init__(self, ADL, path_index):
        self.path_index = path_index
        self.n_path_lengths = len(path_index.path_indices)
        self._buffers = {ADL.path_indices_prefix + str(i): torch.from_numpy(pi) for i, pi in enumerate(path_index.path_indices)}
        self.disp_target = torch.from_numpy(path_index.search_dst).t()[None, :, :, None].float()       # [1, 2, D, 1]: (dy, dx)


def reference_losses(ADL, PathIndex, GetLabels, edge, dp, label, radius):
    """-> (losses [4] tensors, counts [3], edge_out leaf, dp_out leaf)"""
    B, _, h, w = edge.shape
    pi = PathIndex(radius=radius, default_size=(h, w))
    me = StandIn(ADL, pi)
    edge_out = torch.from_numpy(edge).requires_grad_(True)
    dp_out = torch.from_numpy(dp).requires_grad_(True)
    aff = ADL.to_affinity(me, torch.sigmoid(edge_out))
    pair_disp = ADL.to_pair_displacement(me, dp_out)
    # the four per-pair loss maps of the forward (resnet50_irn.py:211-220)
    per_pair = {"pos": -torch.log(aff + 1e-5), "neg": -torch.log(1. + 1e-5 - aff),
                "fg": ADL.to_displacement_loss(me, pair_disp), "bg": pair_disp.abs()}
    # the loader's labels (dataloader.py:90-109), batched as the DataLoader's collate does
    get = GetLabels(pi.src_indices, pi.dst_indices)
    labs = [get(label[b]) for b in range(B)]
    bg_lab, fg_lab, neg_lab = (torch.stack([l[k] for l in labs]) for k in range(3))

    def masked_mean(x, lab, channels=1):
        """sum over the labelled pairs / (channels * their number + 1e-5): the form of every loss line of train_irn.py:57-63"""
        lab_x = lab if x.dim() == lab.dim() else lab.unsqueeze(1)
        n = lab.sum()
        return (x * lab_x).sum() / ((n if channels == 1 else channels * n) + 1e-5)

    pos_aff_loss = masked_mean(per_pair["pos"], bg_lab) / 2 + masked_mean(per_pair["pos"], fg_lab) / 2
    neg_aff_loss = masked_mean(per_pair["neg"], neg_lab)
    dp_fg_loss = masked_mean(per_pair["fg"], fg_lab, 2)
    dp_bg_loss = masked_mean(per_pair["bg"], bg_lab, 2)
    counts = [int(t.to(torch.float64).sum()) for t in (bg_lab, fg_lab, neg_lab)]
    return (pos_aff_loss, neg_aff_loss, dp_fg_loss, dp_bg_loss), counts, edge_out, dp_out


def main():
    import oracle_irn_loss as O
    torch.set_num_threads(8)
    ADL, PathIndex, GetLabels = reference_modules()
    rec = {}
    for i, (B, h, w, radius) in enumerate(O.GOLDEN_SHAPES):
        edge, dp, label = O.inputs(B, h, w)
        l, counts, e, d = reference_losses(ADL, PathIndex, GetLabels, edge, dp, label, radius)
        total_loss = (l[0] + l[1]) / 2 + (l[2] + l[3]) / 2          # train_irn.py:68
        total_loss.backward()
        assert min(counts) > 0, (B, h, w, radius, counts)
        rec.update({f"s{i}_shape": np.asarray([B, h, w, radius], np.int32), f"s{i}_losses": torch.stack(l).detach().numpy(),
                    f"s{i}_counts": np.asarray(counts, np.int64), f"s{i}_d_edge": e.grad.numpy(), f"s{i}_d_dp": d.grad.numpy()})
        print((B, h, w, radius), "losses", rec[f"s{i}_losses"], "counts", counts)
    B, h, w, radius = O.PLATEAU_SHAPE
    edge, dp, label = O.plateau_inputs()
    l, counts, e, d = reference_losses(ADL, PathIndex, GetLabels, edge, dp, label, radius)
    ((l[0] + l[1]) / 2).backward()
    rec.update({"plateau_shape": np.asarray([B, h, w, radius], np.int32), "plateau_losses": torch.stack(l).detach().numpy(),
                "plateau_counts": np.asarray(counts, np.int64), "plateau_d_edge": e.grad.numpy()})
    print("plateau", rec["plateau_losses"], counts)
    assert all(v.dtype in (np.float32, np.int32, np.int64) for v in rec.values())
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 200_000


if __name__ == "__main__":
    main()
