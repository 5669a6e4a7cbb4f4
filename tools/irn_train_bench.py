"""Times one training iteration of IRNet's edge / displacement heads (tris_amd.irn_train) at the training shape of the reference
(irn_batch_size 32, irn_crop_size 512, radius 10): the whole train_step and, separately, the frozen trunk's forward, the heads'
forward + backward, the loss forward + backward and the optimiser step; beside it the torch-on-ROCm restatement of the same
iteration (tests/oracle_irn_train.py on the device: torch convolutions, GroupNorm, interpolate, the loss restatement of
tests/oracle_irn_loss.py, torch.optim.SGD).  Device events around `inner` calls after a warm-up, median of `reps` windows.

    python tools/irn_train_bench.py [--batch 32] [--size 512] [--radius 10] [--no-torch]

Appends one JSON line to profiles/irn_train_bench.jsonl (--out).  Needs the MI355X: there is nothing to time without it.
Not measured here: per-kernel times (a profiler run of its own).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_batch(B, S, seed=0):
    """normalised-looking float images with a zero-padded rim on some, labels with one object per image and an ignored scatter"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, S, S, 3, generator=g)
    img[::3, S - S // 8:, :, :] = 0.0
    h = (S - 1) // 4 + 1
    label = torch.zeros(B, h, h, dtype=torch.uint8)
    for b in range(B):
        y0, x0 = int(torch.randint(0, h // 2, (1,), generator=g)), int(torch.randint(0, h // 2, (1,), generator=g))
        label[b, y0:y0 + h // 3, x0:x0 + h // 3] = 1 + b % 20
        label[b, torch.randint(0, h, (64,), generator=g), torch.randint(0, h, (64,), generator=g)] = 255
    return img, label


def time_ms(fn, reps, inner):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irn_train_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("irn_train_bench needs the MI355X (no GPU in this process)")
    from tris_amd import irn_loss, ops
    from tris_amd.irn_net import EdgeDisplacement
    from tris_amd.irn_train import IrnTrainer
    from tris_amd.utils.synth import irn_fill
    net = EdgeDisplacement()
    irn_fill(net.state_dict(), 0, 1.0)
    start = {k: v.clone() for k, v in net.state_dict().items()}
    net.cuda()
    # a learning rate of 0 keeps the weights where they are over the timed iterations; the launches are the same
    tr = IrnTrainer(net, lr=0.0, weight_decay=1e-4, max_step=1 << 30, radius=a.radius)
    img, label = (t.cuda() for t in make_batch(a.batch, a.size))
    rec = {"shape": [a.batch, a.size, a.size], "radius": a.radius, "arithmetic": ops.get_gemm_mode(),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner}
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = tr.train_step(img, label)
    torch.cuda.synchronize()
    rec["hip_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    rec["losses"] = [float(v) for v in out["losses"].cpu()]
    rec["hip_train_step"] = time_ms(lambda: tr.train_step(img, label), a.reps, a.inner)
    with tr.scope():
        rec["hip_trunk_forward"] = time_ms(lambda: tr.taps(img), a.reps, a.inner)
        taps = tr.taps(img)
        edge_out, dp_out = tr.heads(taps)
        e, d = edge_out.detach().requires_grad_(True), dp_out.detach().requires_grad_(True)

        def loss_step():
            e.grad = d.grad = None
            losses, _ = irn_loss.affinity_displacement_losses(e, d, label, a.radius)
            irn_loss.total_loss(losses).backward()
        rec["hip_loss_fwd_bwd"] = time_ms(loss_step, a.reps, a.inner)
        ge, gd = e.grad.clone(), d.grad.clone()

        def heads_step():
            eo, do = tr.heads(taps)
            torch.autograd.backward([eo, do], [ge, gd])
        rec["hip_heads_fwd_bwd"] = time_ms(heads_step, a.reps, a.inner)
        rec["hip_optimizer_step"] = time_ms(tr.optimizer.step, a.reps, a.inner)
    del taps, edge_out, dp_out, e, d
    if not a.no_torch:
        import oracle_irn as O
        import oracle_irn_loss as L
        import oracle_irn_train as T
        sd = {k: v.cuda() for k, v in start.items() if v.is_floating_point()}
        leaves = {k: sd[k].clone().requires_grad_(True) for names in T.head_names() for k in names}
        edge_n, dp_n = T.head_names()
        opt = torch.optim.SGD([{"params": [leaves[k] for k in edge_n], "lr": 0.0, "weight_decay": 1e-4},
                               {"params": [leaves[k] for k in dp_n], "lr": 0.0, "weight_decay": 1e-4}], 0.0, 1e-4)
        x = img.permute(0, 3, 1, 2).contiguous()

        def torch_step():
            with torch.no_grad():
                taps = [t.detach() for t in O.trunk(x, sd)]
            eo, do, _ = T.heads(leaves, taps)
            losses, _ = L.losses(eo, do, label, a.radius)
            opt.zero_grad()
            L.total(losses).backward()
            opt.step()
            return losses

        try:
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            losses = torch_step()
            torch.cuda.synchronize()
            rec["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            rec["torch_losses"] = [float(v) for v in losses.detach().cpu()]
            rec["torch_train_step"] = time_ms(torch_step, 3, 2)
        except torch.cuda.OutOfMemoryError as err:
            rec["torch_train_step"] = None
            rec["torch_note"] = f"out of memory: {str(err)[:120]}"
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
