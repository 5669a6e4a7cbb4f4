"""Records tests/golden/g17_irn_train.npz from the REAL reference code, on the CPU, in fp32: IRNet's AffinityDisplacementLoss
(IRNet/net/resnet50_irn.py) in train mode and misc.torchutils.PolyOptimizer on the inputs of tests/oracle_irn_train.py.
Build-machine tool: the reference tree is not on the GPU machines, and nothing that runs there reads it.

    python tools/gen_golden_irn_train.py

The stubs are those of tools/gen_golden_irn.py / gen_golden_irn_loss.py: model_zoo.load_url is replaced BEFORE construction (the
load is strict=False), so nothing leaves the machine.  Weights: irn_fill with the seed and gain of g15_irn_net.npz.

Recorded, for the first input seed that meets the conditions below:
 (a) per shape of oracle_irn_train.SHAPES: edge_out, dp_out of model(x, False) after model.train(), and a strided sample of the
     gradient of every head parameter under sum(Ge edge_out) + sum(Gd dp_out);
 (b) for shape STEP_SHAPE: the four losses of step 0 and a strided sample of every head parameter after N_STEPS iterations of
     the training loop (train_irn.py:55-72: the reference's model and PolyOptimizer are called; the loss reductions between them
     are a loop body, not a function, and are written here in this project's own form, masked_mean and oracle_irn_loss.total) with PolyOptimizer (lr LR, weight decay WEIGHT_DECAY, max_step MAX_STEP), pair labels from
     GetAffinityLabelFromIndices; the learning rates PolyOptimizer set, for MAX_STEP + 2 steps of an optimiser of its own;
 (c) the running_mean of train_irn.py:93-106 over two batches (shapes 0 and 2).
Conditions on the seed (checked with the restatement, on the CPU): every label map has a bg, an fg and a neg pair; the fp32
restatement's own ReLU masks differ from the fp64 ones only below 1e-4 of a tensor's rms and at no more than 1e-3 of all elements;
the fp32-to-fp64 distance of the three-step update is below 1e-3 per tensor (near-tied path maxima reroute gradients); if no seed
of the first ten meets the last one, it is dropped and `update_ok` is recorded as 0.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "g17_irn_train.npz")


def reference_model(ADL, PathIndex, radius, hw, seed, gain):
    from tris_amd.utils.synth import irn_fill
    pi = PathIndex(radius=radius, default_size=hw)
    model = ADL(pi).float()
    from tris_amd.irn_net import TRAINING_ONLY
    irn_fill({k: v for k, v in model.state_dict().items() if not TRAINING_ONLY.fullmatch(k)}, seed, gain)
    model.train()
    assert model.training and model.fc_dp7.training and not model.stage1.training and not model.resnet50.layer1.training
    return model, pi


def masked_mean(x, lab, channels=1):
    """sum of x over the labelled pairs / (channels * their number + 1e-5): the form of every loss line of the training loop (the
    helper of tools/gen_golden_irn_loss.py, which keeps it inside a function)"""
    lab_x = lab if x.dim() == lab.dim() else lab.unsqueeze(1)
    n = lab.sum()
    return (x * lab_x).sum() / ((n if channels == 1 else channels * n) + 1e-5)


def seed_conditions(T, L, sd, seed):
    """-> (labels ok, masks ok, update distance fp32 vs fp64 of the three-step run)"""
    for i, (B, H, W, radius) in enumerate(T.SHAPES):
        lab = T.labels(i, seed)
        e, d = T.cotangents(i, seed)
        for b in range(B):
            _, n = L.losses(e[b:b + 1].double(), d[b:b + 1].double(), lab[b:b + 1], radius)
            if int(n.min()) < 1:
                return False, False, None
    for i in range(len(T.SHAPES)):
        x = T.images(i, seed)
        Ge, Gd = T.cotangents(i, seed)
        r32 = T.linear_functional(sd, x, Ge, Gd, torch.float32)
        r64 = T.linear_functional(sd, x, Ge, Gd, torch.float64)
        frac, worst = T.mask_disagreement(T.own_masks(r32["pre"]), r64["pre"])
        print(f"  seed {seed} shape {i}: fp32 masks differ at {frac:.2e} of the elements, largest |pre| / rms among them {worst:.2e}")
        if frac > 1e-3 or worst > 1e-4:
            return True, False, None
    B, H, W, radius = T.SHAPES[T.STEP_SHAPE]
    x, lab = T.images(T.STEP_SHAPE, seed), T.labels(T.STEP_SHAPE, seed)
    _, p32, b32 = T.train_steps(sd, x, lab, radius, torch.float32)
    _, p64, b64 = T.train_steps(sd, x, lab, radius, torch.float64)
    dist = max(T.rel_l2((p32[k] - b32[k]).numpy(), (p64[k] - b64[k]).numpy()) for k in p32)
    print(f"  seed {seed}: fp32-to-fp64 distance of the three-step update, worst tensor {dist:.3e}")
    return True, True, dist


def main():
    import gen_golden_irn_loss as GL
    import oracle_irn as O
    import oracle_irn_loss as L
    import oracle_irn_train as T
    torch.set_num_threads(8)
    ADL, PathIndex, GetLabels = GL.reference_modules()
    from misc.torchutils import PolyOptimizer        # noqa: E402  (the reference's)
    g15 = np.load(os.path.join(ROOT, "tests", "golden", "g15_irn_net.npz"))
    wseed, gain = int(g15["seed"]), float(g15["gain"])
    sd = O.filled_state_dict(wseed, gain)
    edge_names, dp_names = T.head_names()

    chosen, update_ok, fallback = None, 0, None
    for seed in range(10):
        ok_lab, ok_mask, dist = seed_conditions(T, L, sd, seed)
        if not (ok_lab and ok_mask):
            continue
        if fallback is None:
            fallback = seed
        if dist < 1e-3:
            chosen, update_ok = seed, 1
            break
    if chosen is None:
        if fallback is None:
            raise SystemExit("no seed met the label and mask conditions")
        chosen = fallback
    seed = chosen
    print("input seed", seed, "three-step update comparable:", bool(update_ok))
    rec = {"weight_seed": np.int32(wseed), "gain": np.float32(gain), "seed": np.int32(seed), "update_ok": np.int32(update_ok)}

    # ---- (a) forward and the gradients of the linear functional
    for i, (B, H, W, radius) in enumerate(T.SHAPES):
        model, _ = reference_model(ADL, PathIndex, radius, T.map_size(H, W), wseed, gain)
        named = dict(model.named_parameters())
        x = T.images(i, seed)
        Ge, Gd = T.cotangents(i, seed)
        edge_out, dp_out = model(x, False)
        assert tuple(edge_out.shape) == (B, 1) + T.map_size(H, W) and tuple(dp_out.shape) == (B, 2) + T.map_size(H, W)
        ((Ge * edge_out).sum() + (Gd * dp_out).sum()).backward()
        rec[f"a{i}_edge_out"], rec[f"a{i}_dp_out"] = edge_out.detach().numpy(), dp_out.detach().numpy()
        for k in edge_names + dp_names:
            rec[f"a{i}_grad_{k}"] = T.sample(named[k].grad).numpy().copy()
        assert all(p.grad is None for k, p in named.items() if k.startswith("resnet50."))

    # ---- (b) three iterations of the reference's loop
    B, H, W, radius = T.SHAPES[T.STEP_SHAPE]
    model, pi = reference_model(ADL, PathIndex, radius, T.map_size(H, W), wseed, gain)
    named = dict(model.named_parameters())
    groups = model.trainable_parameters()
    assert [id(p) for p in groups[0]] == [id(named[k]) for k in edge_names]
    assert [id(p) for p in groups[1]] == [id(named[k]) for k in dp_names]
    opt = PolyOptimizer([{"params": groups[0], "lr": 1 * T.LR, "weight_decay": T.WEIGHT_DECAY},
                         {"params": groups[1], "lr": 10 * T.LR, "weight_decay": T.WEIGHT_DECAY}],
                        lr=T.LR, weight_decay=T.WEIGHT_DECAY, max_step=T.MAX_STEP)
    x, lab = T.images(T.STEP_SHAPE, seed), T.labels(T.STEP_SHAPE, seed).numpy()
    get = GetLabels(pi.src_indices, pi.dst_indices)
    labs = [get(lab[b]) for b in range(B)]
    bg_lab, fg_lab, neg_lab = (torch.stack([l[k] for l in labs]) for k in range(3))
    for step in range(T.N_STEPS):
        maps = dict(zip(("pos", "neg", "fg", "bg"), model(x, True)))          # the reference's four per-pair loss maps
        losses = [masked_mean(maps["pos"], bg_lab) / 2 + masked_mean(maps["pos"], fg_lab) / 2, masked_mean(maps["neg"], neg_lab),
                  masked_mean(maps["fg"], fg_lab, 2), masked_mean(maps["bg"], bg_lab, 2)]
        if step == 0:
            rec["b_losses"] = torch.stack(losses).detach().numpy()
        for p in named.values():
            p.grad = None
        L.total(losses).backward()
        opt.step()
        print("step", step, "losses", [float(v) for v in losses], "lr", [g["lr"] for g in opt.param_groups])
    for k in edge_names + dp_names:
        rec[f"b_param_{k}"] = T.sample(named[k].detach()).numpy().copy()
        assert np.isfinite(rec[f"b_param_{k}"]).all(), k
    rec["b_momentum"] = np.float64(opt.param_groups[0]["momentum"])
    rec["b_group_wd"] = np.asarray([g["weight_decay"] for g in opt.param_groups], np.float64)
    # the schedule, from an optimiser of its own on a scalar parameter (zero gradient: only the learning rates are read)
    q = torch.nn.Parameter(torch.zeros(1))
    sched = PolyOptimizer([{"params": [q], "lr": 1 * T.LR, "weight_decay": T.WEIGHT_DECAY}], lr=T.LR, weight_decay=T.WEIGHT_DECAY,
                          max_step=T.MAX_STEP)
    q.grad = torch.zeros(1)
    lrs = []
    for _ in range(T.MAX_STEP + 2):
        sched.step()
        lrs.append(sched.param_groups[0]["lr"])
    rec["b_lr_sequence"] = np.asarray(lrs, np.float64)

    # ---- (c) the mean shift over two batches: eval mode, the per-channel mean of dp_out of every batch, then their mean
    batch_means = []
    for i in (0, 2):
        B, H, W, radius = T.SHAPES[i]
        model, _ = reference_model(ADL, PathIndex, radius, T.map_size(H, W), wseed, gain)
        model.eval()
        rec["c_start"] = model.mean_shift.running_mean.numpy().copy()
        with torch.no_grad():
            dp_out = model(T.images(i, seed), False)[1]
        batch_means.append(dp_out.mean(dim=(0, 2, 3)))
    rec["c_running_mean"] = torch.stack(batch_means).mean(dim=0).numpy()

    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    main()
