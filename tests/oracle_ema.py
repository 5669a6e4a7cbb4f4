"""TEST INFRASTRUCTURE ONLY -- CPU restatements for Stage-2 EMA consistency training (train_stage2.py:58-63, 258-269, 302-332):
the schedule and update rule of ema_pytorch.EMA 0.2.3 at its defaults as DESIGN section 16 states them (on dicts of tensors, in
fp64), sigmoid_mse_loss and the six losses, and the teacher's forward -- trunk on running statistics, decoder on batch statistics --
composed from tests/oracle_stage2.py.  The package itself is on no machine of this project: this file restates the same written
rule independently of tris_amd/ema.py, it is not a comparison with the package."""
import torch
import torch.nn.functional as F

import oracle_stage2 as S
from oracle import tris_oracle as O


def current_decay(step, beta=0.9999, update_after_step=100, inv_gamma=1.0, power=2 / 3, min_value=0.0):
    """get_current_decay() for the ALREADY INCREMENTED step counter"""
    epoch = max(step - update_after_step - 1, 0)
    if epoch <= 0:
        return 0.0
    return min(max(1 - (1 + epoch / inv_gamma) ** -power, min_value), beta)


class Schedule:
    """the host side of update(): call -> list of actions of this update, each ("copy",) or ("lerp", decay)"""

    def __init__(self, beta=0.9999, update_after_step=100, update_every=10, inv_gamma=1.0, power=2 / 3, min_value=0.0):
        self.kw = dict(beta=beta, update_after_step=update_after_step, inv_gamma=inv_gamma, power=power, min_value=min_value)
        self.update_every, self.step, self.initted = update_every, 0, False

    def __call__(self):
        step = self.step
        self.step += 1
        if step % self.update_every != 0:
            return []
        if step <= self.kw["update_after_step"]:
            return [("copy",)]
        acts = []
        if not self.initted:
            acts.append(("copy",))
            self.initted = True
        acts.append(("lerp", current_decay(self.step, **self.kw)))
        return acts


def covered(sd):
    """names update() writes: floating-point tensors only (num_batches_tracked is int64)"""
    return [k for k, v in sd.items() if v.is_floating_point()]


def apply(teacher, student, acts):
    """teacher / student: dicts name -> fp64 tensor; in place on teacher.  lerp_(student, 1 - decay) with the weight the kernel
    receives: the fp32 rounding of the Python double 1 - decay"""
    for a in acts:
        for k in covered(teacher):
            if a[0] == "copy":
                teacher[k].copy_(student[k])
            else:
                w = float(torch.tensor(1.0 - a[1], dtype=torch.float64).float())
                teacher[k].add_(w * (student[k] - teacher[k]))


def sigmoid_mse_loss(x, e):
    """train_stage2.py:258-269"""
    return F.mse_loss(torch.sigmoid(x), torch.sigmoid(e), reduction="mean")


def losses6(outs, ema_outs, target):
    """(l1 + l2 + l3 + l4 + l5, l1, l2, l3, l4, l5) (:302-319); absent heads (None) contribute nothing"""
    ls = [F.binary_cross_entropy_with_logits(o, target.to(o.dtype), reduction="mean") for o in outs if o is not None]
    ls += [torch.zeros((), dtype=ls[0].dtype)] * (4 - len(ls))
    l5 = sum(sigmoid_mse_loss(o, e.detach()) for o, e in zip(outs, ema_outs) if o is not None)
    return [ls[0] + ls[1] + ls[2] + ls[3] + l5] + ls + [l5]


def teacher_forward(sd, img, ids):
    """the EMA copy's forward as train_stage2.py builds it (:58-63): root and decoder in train mode, `backbone` in eval mode.
    -> four maps; the decoder's running statistics in `sd` are updated in place, as the module's are"""
    c1, c2, c3, c4 = O.encode_image_rn(sd, "backbone.", img, False)
    words, _ = O.encode_text(sd, "backbone.", ids)
    lan = words.permute(0, 2, 1)
    f2 = O.pixel_attention(sd, "attention2", c2, lan) + c2
    f3 = O.pixel_attention(sd, "attention3", c3, lan) + c3
    f4 = O.pixel_attention(sd, "attention4", c4, lan) + c4
    dem1, dem2 = S.cbr(sd, "reduced_c1", c1, True), S.cbr(sd, "reduced_c2", f2, True)
    dem3, dem4 = S.cbr(sd, "reduced_c3", f3, True), S.cbr(sd, "reduced_c4", f4, True)
    s4 = S.up(S.cbr(sd, "output4", dem4, True), dem3.shape[2:])
    s3 = S.up(S.cbr(sd, "output3", s4 + dem3, True), dem2.shape[2:])
    s2 = S.up(S.cbr(sd, "output2", s3 + dem2, True), dem1.shape[2:])
    s1 = S.cbr(sd, "output1", s2 + dem1, True)
    size = img.shape[2:]
    S.head.train = True
    return (S.head(sd, "final_seg1", s1, size), S.head(sd, "final_seg2", s2, size), S.head(sd, "final_seg3", s3, size),
            S.head(sd, "final_seg4", s4, size))
