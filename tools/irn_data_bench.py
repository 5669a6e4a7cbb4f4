"""Times IRNet's training input pipeline (tris_amd.dataset.irn_data, csrc/irndata.hip) at the training shape of the reference
(irn_batch_size 32, irn_crop_size 512, rescale (0.5, 1.5)) on synthetic sources of COCO's usual sizes, 640x480 and 480x640:

  (a) the augment launch per batch: device events around `inner` launches on prepared descriptors, after a warm-up
  (b) the host side per batch, IrnLoader.prepare: the draw, the table build, the checks and the one copy (host clock, no
      launch); the table build and the checks also on their own
  (c) the training loop (IrnTrainer.train_step, learning rate 0 as tools/irn_train_bench.py) fed by the loader against the same
      loop on one fixed, pre-made batch, one after the other: images per second, host clock around synchronised windows
  (d) the same transform by Pillow and numpy on the host, per image, as the reference's DataLoader worker does it
      (tests/oracle_irn_data.py; the decode is not in it)
Every figure is the median of `reps` windows with their minimum and maximum.

    python tools/irn_data_bench.py [--batch 32] [--crop 512] [--images 64] [--no-train]

Appends one JSON line to profiles/irn_data_bench.jsonl (--out).  Needs the MI355X.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


class ArrayData:
    """the index HbmIrnCache asks for, over arrays instead of files"""

    def __init__(self, images, labels, crop_size):
        self.images, self.labels, self.crop_size = images, labels, crop_size
        self.rescale, self.hor_flip = (0.5, 1.5), True

    def __len__(self):
        return len(self.images)

    def image_id(self, i):
        return str(i)

    def load_image(self, i):
        return self.images[i]

    def load_label(self, i, size=None):
        return self.labels[i]

    def params(self, rng, H, W):
        from tris_amd.dataset.irn_data import IrnAugParams
        return IrnAugParams.draw(rng, H, W, self.crop_size, self.rescale, self.hor_flip)


def sources(n, seed=0):
    rng = np.random.default_rng(seed)
    images, labels = [], []
    for i in range(n):
        H, W = (480, 640) if i % 2 == 0 else (640, 480)
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.stack([128 + 100 * np.sin(yy / (19.0 + c) + i) * np.cos(xx / (23.0 + i % 7)) for c in range(3)], 2)
        images.append(np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8))
        lab = np.zeros((H, W), np.uint8)
        lab[H // 4:H // 4 + H // 2, W // 3:W // 3 + W // 3] = 1 + i % 20
        lab[rng.integers(0, H, 400), rng.integers(0, W, 400)] = 255
        labels.append(lab)
    return images, labels


def stats(v, key="ms"):
    return {f"median_{key}": statistics.median(v), f"min_{key}": min(v), f"max_{key}": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--steps", type=int, default=6, help="training steps per window of (c)")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irn_data_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("irn_data_bench needs the MI355X (no GPU in this process)")
    import oracle_irn_data as O
    from tris_amd import ops
    from tris_amd.dataset import irn_data as D
    B, crop = a.batch, a.crop
    images, labels = sources(a.images)
    cache = D.HbmIrnCache(ArrayData(images, labels, crop), "cuda")
    loader = D.IrnLoader(cache, B, seed=0)
    rec = {"shape": [B, crop, crop], "images": a.images, "cache_bytes": cache.nbytes, "device": torch.cuda.get_device_name(0),
           "reps": a.reps, "inner": a.inner}

    # (a) the launch alone, on prepared descriptors (a different batch per launch)
    packed = []
    for k in range(a.inner):
        idx = [(k * B + j) % len(cache) for j in range(B)]
        desc, tables = D.build_batch([cache.sample(i) for i in idx], loader.draw(idx), crop)
        D.validate_batch(desc, tables, crop, cache.img_arena.numel() - D.ARENA_SLACK, cache.lab_arena.numel())
        buf = torch.from_numpy(np.concatenate([desc.reshape(-1).view(np.uint8), tables.view(np.uint8)])).cuda()
        packed.append((buf, desc.size * 8))
    rec["table_bytes_per_batch"] = int(packed[0][0].numel())

    def launches():
        for buf, nd in packed:
            ops.irn_augment_batch(cache.img_arena, cache.lab_arena, buf, nd, cache.lut, B, crop)
    launches()
    torch.cuda.synchronize()
    t = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launches()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / a.inner)
    rec["augment_launch"] = stats(t)
    rec["bytes_written_per_batch"] = B * crop * crop * 13 + B * (crop // 4) ** 2

    # (b) the host side per batch: IrnLoader.prepare, and its two large parts timed on their own
    limits = (cache.img_arena.numel() - D.ARENA_SLACK, cache.lab_arena.numel())
    t, t_build, t_check = [], [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.inner):
            idx = [(k * B + j) % len(cache) for j in range(B)]
            loader.prepare(idx, loader.draw(idx))
        t.append((time.perf_counter() - t0) * 1e3 / a.inner)
        torch.cuda.synchronize()
        batches_ = []
        for k in range(a.inner):
            idx = [(k * B + j) % len(cache) for j in range(B)]
            batches_.append(([cache.sample(i) for i in idx], loader.draw(idx)))
        t0 = time.perf_counter()
        built = [D.build_batch(smp, prm, crop) for smp, prm in batches_]
        t1 = time.perf_counter()
        for desc, tables in built:
            D.validate_batch(desc, tables, crop, *limits)
        t2 = time.perf_counter()
        t_build.append((t1 - t0) * 1e3 / a.inner)
        t_check.append((t2 - t1) * 1e3 / a.inner)
    rec["host_per_batch"] = stats(t)
    rec["host_build_tables"] = stats(t_build)
    rec["host_validate"] = stats(t_check)

    # (d) Pillow and numpy on the host, per image
    rng = random.Random(2)
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for i in range(8):
            d = O.draw(rng, images[i].shape[0], images[i].shape[1], crop)
            O.apply(images[i], labels[i], d, crop)
        t.append((time.perf_counter() - t0) * 1e3 / 8)
    rec["pillow_per_image"] = stats(t)

    # (c) the training loop fed by the loader, and on one fixed batch
    if not a.no_train:
        from tris_amd.irn_net import EdgeDisplacement
        from tris_amd.irn_train import IrnTrainer
        from tris_amd.utils.synth import irn_fill
        net = EdgeDisplacement()
        irn_fill(net.state_dict(), 0, 1.0)
        tr = IrnTrainer(net.cuda(), lr=0.0, weight_decay=1e-4, max_step=1 << 30, radius=10)
        rec["arithmetic"] = ops.get_gemm_mode()
        fixed = next(iter(loader))

        def batches():
            while True:
                yield from loader

        feed = batches()

        def window(from_loader):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                img, _, red = next(feed) if from_loader else fixed
                tr.train_step(img, red)
            torch.cuda.synchronize()
            return a.steps * B / (time.perf_counter() - t0)

        for from_loader in (False, True):          # warm-up of both forms
            window(from_loader)
        rec["loop_fixed_batch"] = stats([window(False) for _ in range(a.reps)], "img_s")
        rec["loop_from_loader"] = stats([window(True) for _ in range(a.reps)], "img_s")
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
