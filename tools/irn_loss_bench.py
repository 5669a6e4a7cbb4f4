"""Times IRNet's affinity / displacement training losses (tris_amd.irn_loss, csrc/irnloss.hip), forward + backward, at the training
shape of the reference (irn_batch_size 32, irn_crop_size 512 / 4 = 128 x 128 maps, radius 10), and the torch-on-ROCm
restatement of the same contract (tests/oracle_irn_loss.py: one index_select + max_pool2d per path length, as the reference's
AffinityDisplacementLoss.to_affinity; it derives the pair labels on the device where the reference's loader does it on the
host).  Device events around `inner` calls, median of `reps`; both compute the same input, and the run compares their results.

    python tools/irn_loss_bench.py [--batch 32] [--size 128] [--radius 10] [--no-torch]

Appends one JSON line to profiles/irn_loss_bench.jsonl (--out).  Needs the MI355X: there is nothing to time without it.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_inputs(B, h, w, seed=0):
    """network-like maps: smooth-ish logits, displacements of a few pixels, labels with one object per image and an ignored rim"""
    g = torch.Generator().manual_seed(seed)
    edge = torch.randn(B, 1, h, w, generator=g) * 2.0 - 1.0
    dp = torch.randn(B, 2, h, w, generator=g) * 3.0
    label = torch.zeros(B, h, w, dtype=torch.uint8)
    for b in range(B):
        y0, x0 = int(torch.randint(0, h // 2, (1,), generator=g)), int(torch.randint(0, w // 2, (1,), generator=g))
        label[b, y0:y0 + h // 3, x0:x0 + w // 3] = 1 + b % 20
        label[b, torch.randint(0, h, (64,), generator=g), torch.randint(0, w, (64,), generator=g)] = 255
    return edge, dp, label


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
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irn_loss_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("irn_loss_bench needs the MI355X (no GPU in this process)")
    from tris_amd import irn, irn_loss
    B, h, w = a.batch, a.size, a.size
    edge, dp, label = (t.cuda() for t in make_inputs(B, h, w))
    e, d = edge.clone().requires_grad_(True), dp.clone().requires_grad_(True)

    def hip_fwd():
        with torch.no_grad():
            return irn_loss.affinity_displacement_losses(edge, dp, label, a.radius)

    def hip_step():
        e.grad = d.grad = None
        losses, counts = irn_loss.affinity_displacement_losses(e, d, label, a.radius)
        irn_loss.total_loss(losses).backward()
        return losses, counts

    losses, counts = hip_step()
    n_dirs = len(irn.search_dirs(a.radius))
    n_cells = sum(len(c) for _, c in irn.search_paths(a.radius))
    rec = {"shape": [B, h, w], "radius": a.radius, "n_dirs": n_dirs, "pairs": int(counts.sum()),
           "pairs_possible": B * n_dirs * (h - a.radius + 1) * (w - 2 * a.radius + 2), "path_cells_per_source": n_cells,
           "losses": [float(v) for v in losses.detach().cpu()], "counts": counts.cpu().tolist(),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner}
    rec["hip_fwd_ms"], rec["hip_fwd_min_ms"], rec["hip_fwd_max_ms"] = time_ms(hip_fwd, a.reps, a.inner)
    rec["hip_fwd_bwd_ms"], rec["hip_fwd_bwd_min_ms"], rec["hip_fwd_bwd_max_ms"] = time_ms(hip_step, a.reps, a.inner)
    ge, gd = e.grad.clone(), d.grad.clone()
    if not a.no_torch:
        import oracle_irn_loss as O
        te, td = edge.clone().requires_grad_(True), dp.clone().requires_grad_(True)

        def torch_step():
            te.grad = td.grad = None
            l, n = O.losses(te, td, label, a.radius)
            O.total(l).backward()
            return l, n

        try:
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            l, n = torch_step()
            torch.cuda.synchronize()
            rec["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            rec["torch_fwd_bwd_ms"], rec["torch_fwd_bwd_min_ms"], rec["torch_fwd_bwd_max_ms"] = time_ms(torch_step, 3, 3)
            rec["torch_losses"] = [float(v) for v in l.detach().cpu()]
            rec["d_edge_rel_l2_vs_torch"] = float((ge - te.grad).norm() / te.grad.norm())
            rec["d_dp_rel_l2_vs_torch"] = float((gd - td.grad).norm() / td.grad.norm())
        except torch.cuda.OutOfMemoryError as err:
            rec["torch_fwd_bwd_ms"] = None
            rec["torch_note"] = f"out of memory: {str(err)[:120]}"
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
