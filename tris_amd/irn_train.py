"""Training IRNet's edge / displacement heads on the MI355X: the loop body of the reference's IRNet/step_refer/train_irn.py:55-72 and
its closing mean-shift pass (:93-106) on this stack.

    net = EdgeDisplacement(); net.load_state_dict(backbone_and_initial_heads); net.cuda()
    trainer = IrnTrainer(net, lr=0.1, weight_decay=1e-4, max_step=n_steps)
    for img, label in batches:                       # img float32 [B,3,H,W] normalised, label uint8 [B,H,W] (or at the maps' size)
        out = trainer.train_step(img, label)         # {'losses' [4], 'total', 'counts' [3]}: device tensors, no host sync
    trainer.fit_mean_shift(eval_batches)
    torch.save(trainer.state_dict(), path)           # the file `python -m tris_amd.make_ins_seg --irn_weights_name` takes

The reference detaches every trunk tap (IRNet/net/resnet50_irn.py:117-121) and keeps the backbone in eval mode (:145-147): the
ResNet-50 runs forward only, under no_grad, on the inference kernels of tris_amd.irn_net behind a float stem; fc_edge1..6 and
fc_dp1..7 train (IrnHeadsFn below, csrc/irntrain.hip), the loss is tris_amd.irn_loss, the optimiser tris_amd.optim.PolySGD.
IrnHeadsFn lives here and not in irn_net because only training needs a backward: its forward is irn_net.run_heads, the one
inference runs, and its backward walks irn_net's branch tables.
Train-mode semantics: MeanShift is the identity (:111-114), there is no flip-average.  There is no CPU path: ops.NoGpuError.
The dataset, its augmentation and the command line: tris_amd.dataset.irn_data, tris_amd.train_irn.
Not here: the CRF labels, data parallelism, graph capture of the step.
"""
import contextlib

import torch

from . import irn_loss, ops
from .irn_net import GROUPS, EdgeDisplacement, branch_names, head_parameter_names, run_heads
from .optim import PolySGD

N_TAPS = 5
HEAD_NAMES = tuple(n for names in head_parameter_names() for n in names)      # the order IrnHeadsFn takes the parameters in


def _wgrad_1x1(p, dt, x, needs):
    """dW [N,K] = dt^T x for a 1x1 convolution weight, on the dense-product path; into the parameter's arena view if it has one"""
    N, K = dt.shape[-1], x.shape[-1]
    M = x.numel() // K
    return ops._emit(p, lambda o: ops.gemm(dt, x, o, N, K, M, N, K, K, True, False, mark=False), needs)


def _dgrad_1x1(dt, w):
    """dX [M,K] = dt w for a 1x1 convolution weight [N,K,1,1]"""
    N = dt.shape[-1]
    K = w.numel() // N
    M = dt.numel() // N
    dx = torch.empty(*dt.shape[:-1], K, dtype=torch.float32, device=dt.device)
    ops.gemm(dt, w, dx, M, K, N, N, K, K, False, False, w_b=True, w_bt=True)
    return dx


def _backward_order(branches, head):
    """the branches in an order that has every buffer's gradient complete before a branch that wrote into it runs: buffer by
    buffer from the head's, each buffer's writers in table order, a buffer that a branch reads queued behind"""
    queue = [head.src]
    for buf in queue:
        for b in branches:
            if b.dst == buf:
                yield b
                if not isinstance(b.src, int):
                    queue.append(b.src)


class IrnHeadsFn(torch.autograd.Function):
    """Net.forward's two branches in train mode (irn_net.run_heads without a dp bias): taps x1..x5 (channels-last, detached) and
    the head parameters in HEAD_NAMES order -> edge_out [B,1,h,w], dp_out [B,2,h,w].  The Function owns the concatenation buffers,
    the GroupNorm inputs and their statistics, and runs the backward in one fixed order; the only data gradients formed are those
    of the branches that read a buffer (fc_dp7's and fc_dp6's inputs; no tap has one)."""

    @staticmethod
    def forward(ctx, keep, *args):
        taps, prm = args[:N_TAPS], args[N_TAPS:]
        if len(prm) != len(HEAD_NAMES):
            raise ValueError(f"IrnHeadsFn takes {len(HEAD_NAMES)} parameters, got {len(prm)}")
        ops._chk(*taps, *prm)
        ctx.taps, ctx.prm, ctx.rec = [t.contiguous() for t in taps], dict(zip(HEAD_NAMES, prm)), {}
        y = run_heads(ctx.taps, ctx.prm, record=ctx.rec)
        if keep is not None:
            keep.update({k: v for k, v in ctx.rec.items() if k != "gn"})
        return tuple(y[k].permute(0, 3, 1, 2).contiguous() for k in GROUPS)      # (no copy of the one-channel edge map)

    @staticmethod
    def backward(ctx, *g_out):
        taps, prm, rec = ctx.taps, ctx.prm, ctx.rec
        need = dict(zip(HEAD_NAMES, ctx.needs_input_grad[1 + N_TAPS:]))
        if any(ctx.needs_input_grad[1:1 + N_TAPS]):
            raise RuntimeError("irn_heads: the taps are detached in the reference (resnet50_irn.py:117-121); they take no gradient")
        out = dict.fromkeys(HEAD_NAMES)

        def emit(name, value, sink):
            """a gradient the kernel wrote: None to autograd when it went into the parameter's arena view or is not asked for"""
            out[name] = value.view_as(prm[name]) if sink is None and need[name] else None

        for (branches, head), g in zip(GROUPS.values(), g_out):
            x = rec[head.src]
            if g is None:
                g = torch.zeros(x.shape[0], head.cout, *x.shape[1:3], dtype=torch.float32, device=x.device)
            wn, bn = f"{head.name}.weight", f"{head.name}.bias"
            sw, sb = ops._sink(prm[wn]), ops._sink(prm[bn]) if head.bias else None
            d_x, dw, db = ops.irn_head_bwd(g.permute(0, 2, 3, 1).contiguous(), x, prm[wn].reshape(head.cout, head.cin),
                                           want_db=head.bias, dw=sw, db=sb)
            emit(wn, dw, sw)
            if head.bias:
                emit(bn, db, sb)
            d = {head.src: d_x}                    # buffer -> its gradient
            for b in _backward_order(branches, head):
                conv, gamma, beta = branch_names(b)
                t, st = rec["gn"][b.name]
                sg, sb = ops._sink(prm[gamma]), ops._sink(prm[beta])
                dt, dgam, dbet = ops.gn_up_bwd(d[b.dst], rec[b.dst], b.off, t, st, prm[gamma], b.groups, b.scale,
                                               dgamma=sg, dbeta=sb)
                out[conv] = _wgrad_1x1(prm[conv], dt, taps[b.src] if isinstance(b.src, int) else rec[b.src], need[conv])
                emit(gamma, dgam, sg)
                emit(beta, dbet, sb)
                if not isinstance(b.src, int):
                    d[b.src] = _dgrad_1x1(dt, prm[conv])
        return (None,) * (1 + N_TAPS) + tuple(out[n] for n in HEAD_NAMES)


class IrnTrainer:
    """IrnTrainer(net, lr, weight_decay, max_step, radius=10): the reference's two parameter groups (edge at 1 x lr, dp at 10 x lr,
    train_irn.py:32-36) become trainable, everything else stays frozen."""

    def __init__(self, net, lr, weight_decay, max_step, radius=10):
        if not isinstance(net, EdgeDisplacement):
            raise TypeError(f"IrnTrainer takes a tris_amd.irn_net.EdgeDisplacement, got {type(net).__name__}")
        self.net, self.radius = net, int(radius)
        named = dict(net.named_parameters())
        edge, dp = head_parameter_names()
        for p in named.values():
            p.requires_grad_(False)
        self.edge_params = [named[k].requires_grad_(True) for k in edge]
        self.dp_params = [named[k].requires_grad_(True) for k in dp]
        self.optimizer = PolySGD([{"params": self.edge_params, "lr": 1 * lr, "weight_decay": weight_decay},
                                  {"params": self.dp_params, "lr": 10 * lr, "weight_decay": weight_decay}],
                                 lr=lr, weight_decay=weight_decay, max_step=max_step)
        net._prep = None       # (the parameters moved into the optimiser's arenas: the load-time views are formed again)

    # ------------------------------------------------------------------------------------------------------------- pieces
    @contextlib.contextmanager
    def scope(self, explicit=False):
        """what every pass over the network runs inside -- train_step, eval_outputs, and a caller of the pieces taps() / heads():
        the cost model's tile choice (image sizes change from batch to batch) and one h2 step (ops.h2_step)"""
        with ops.autotune_off(), ops.h2_step(explicit):
            yield

    def _input(self, img):
        if not isinstance(img, torch.Tensor) or img.dtype != torch.float32 or img.dim() != 4 or 3 not in (img.shape[1], img.shape[3]):
            what = f"{tuple(img.shape)} {img.dtype}" if isinstance(img, torch.Tensor) else type(img).__name__
            raise ValueError(f"IrnTrainer takes a float32 image batch [B,3,H,W] or [B,H,W,3], got {what}")
        dev = self.net.fc_edge6.weight.device
        if not torch.cuda.is_available() or dev.type != "cuda":
            raise ops.NoGpuError("tris_amd.irn_train runs on MI355X only (move the network to the GPU); there is no CPU fallback")
        img = img.to(dev)
        if img.shape[3] != 3:
            img = img.permute(0, 2, 3, 1)
        return img.contiguous()

    @torch.no_grad()
    def taps(self, img):
        """the frozen trunk on a normalised float batch -> [x1 .. x5], channels-last"""
        net = self.net
        img = self._input(img)
        p = net._prepare(img.device)
        r = net.resnet50
        y = ops.irn_stem_batch(img, p["stem_w"], r.bn1.running_mean, p["inv"][r.bn1], r.bn1.weight, r.bn1.bias)
        return net._trunk(ops.maxpool3s2(y))

    def heads(self, taps, keep=None):
        """the two branches in train mode -> (edge_out [B,1,h,w], dp_out [B,2,h,w]), differentiable in the head parameters.
        keep: a dict that receives the forward's buffers (cat_e, cat6, cat7, a7: their signs are the ReLU masks).
        As with the project's other arena-backed ops, the backward reads the parameters as they are THEN (autograd is not told of
        an in-place update between forward and backward: do not step in between), and a parameter whose gradient has an arena
        view gets it OVERWRITTEN, not accumulated: a second backward before the optimiser's step replaces the first."""
        return IrnHeadsFn.apply(keep, *taps, *self.edge_params, *self.dp_params)

    def _label(self, label, hw):
        if not isinstance(label, torch.Tensor) or label.dtype != torch.uint8 or label.dim() != 3:
            what = f"{tuple(label.shape)} {label.dtype}" if isinstance(label, torch.Tensor) else type(label).__name__
            raise ValueError(f"IrnTrainer.train_step takes a uint8 label [B,H,W], got {what}")
        label = label.to(self.net.fc_edge6.weight.device)
        if tuple(label.shape[1:]) != tuple(hw):
            label = irn_loss.reduce_label(label)
            if tuple(label.shape[1:]) != tuple(hw):
                raise ValueError(f"IrnTrainer.train_step: the label reduces to {tuple(label.shape[1:])}, the maps are {tuple(hw)}")
        return label.contiguous()

    # --------------------------------------------------------------------------------------------------------------- step
    def train_step(self, img, label):
        """one iteration of train_irn.py:55-72 -> {'losses' [4] = (pos_aff, neg_aff, dp_fg, dp_bg), 'total', 'counts' int64 [3]},
        detached device tensors (no host sync)"""
        img = self._input(img)
        with self.scope(explicit=True):      # one amax pool for the step; the arenas' weights get their amaxes at its start
            taps = self.taps(img)
            edge_out, dp_out = self.heads(taps)
            label = self._label(label, edge_out.shape[2:])
            losses, counts = irn_loss.affinity_displacement_losses(edge_out, dp_out, label, self.radius)
            total = irn_loss.total_loss(losses)
            self.optimizer.zero_grad()
            total.backward()
            self.optimizer.step()
        return {"losses": losses.detach(), "total": total.detach(), "counts": counts}

    # --------------------------------------------------------------------------------------------------------- mean shift
    @torch.no_grad()
    def eval_outputs(self, img):
        """the eval-mode batched forward, model(img, False) of train_irn.py:102: (edge_out [B,1,h,w], dp_out [B,2,h,w]) with the
        current mean shift subtracted (resnet50_irn.py:114)"""
        img = self._input(img)
        with self.scope():
            edge_out, dp_out = self.heads(self.taps(img))
        return edge_out, dp_out - self.net.mean_shift.running_mean.view(1, 2, 1, 1)

    @torch.no_grad()
    def fit_mean_shift(self, batches):
        """train_irn.py:93-106: mean(dp, dim=(0, 2, 3)) of every batch, their mean -> mean_shift.running_mean; returns it"""
        means = [torch.mean(self.eval_outputs(img)[1], dim=(0, 2, 3)) for img in batches]
        if not means:
            raise ValueError("fit_mean_shift: no batches")
        self.net.mean_shift.running_mean.copy_(torch.mean(torch.stack(means), dim=0))
        return self.net.mean_shift.running_mean

    def state_dict(self):
        """the network's tensors under canonical names, on the CPU: what EdgeDisplacement.load_state_dict loads"""
        return {k: v.detach().cpu().clone() for k, v in self.net.state_dict().items()}
