"""Stage-2 training throughput on one MI355X: img/s and ms/step of eager train_stage2.train_step at B = 48, 320 px, T = 20, in
both arithmetics of the dense products (h2, x3).  Seed-filled weights, synthetic images / tokens / pseudo targets.

    python tools/stage2_bench.py [--steps 20] [--warmup 5] [--batch 48] [--loader synthetic|dataloader|hbm] [--arith h2,x3]
                                 [--model_ema]

Prints one JSON line per arithmetic.  No target is set; the FLOP count it assumes is printed with it (forward, per image:
the trunk + text encoder of Stage-1 plus the decoder and the three PixelAttentions, computed from the shapes).

--model_ema: the step with EMA consistency training (tris_amd.ema.EMA built and bound as train_stage2.main does: the teacher's
no-grad forward, ops.seg_loss5, and the teacher update every tenth step); the JSON line carries "model_ema": true and l5.

--loader synthetic (default): one batch already on the device, stepped over and over -- what the step itself costs.
--loader dataloader | hbm: the steps of train_stage2.train_one_epoch fed by the loader the trainer builds under TRIS_HBM_LOADER=0 |
the default (DataLoader(num_workers=2, pin_memory=True, shuffle=True) | tris_amd.dataset.hbm), epoch after epoch over a synthetic
dataset on disk (utils.synth.make_mini_refer at the COCO sizes 480x640, 427x640, 640x480 with make_pseudo_masks, word_hash_tokenize)
until --steps steps (default 300) are timed behind the warm-up, with one device synchronise at the end.  Only full batches are
drawn, and the DataLoader keeps its two workers across the short epochs.  Building the HBM cache is timed separately
(cache_build_s, cache_bytes; 0 for the DataLoader).
Caveat: the synthetic images are PNG-encoded, which decodes faster than the JPEGs of the real dataset, so the `dataloader` leg
underestimates what decoding costs a real run -- the error is in that leg's favour."""
import argparse
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("TRIS_RANDOM_INIT", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

DECODER_GFLOP = 9.2      # the twelve 3x3 convolutions + heads, per image forward at 320 px (computed from the shapes)
PIXATTN_GFLOP = 10.1     # attention2..4 at 40^2 / 20^2 / 10^2, T = 20


def _fed_loader(kind, root, batch, size=320):
    """-> (loader of full training batches with pseudo_gt, cache build seconds, cache bytes)"""
    from torch.utils.data import DataLoader
    from tris_amd.dataset.hbm import HbmLoader, HbmReferCache
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.transform import get_transform
    from tris_amd.utils.synth import word_hash_tokenize
    ds = ReferDataset(root, "refcocog", "umd", image_transforms=get_transform(size, True), split="train", eval_mode=False,
                      size=size, max_tokens=20, pseudo_path=os.path.join(root, "pseudo"), tokenizer=word_hash_tokenize)
    if len(ds) < batch:
        raise ValueError(f"{len(ds)} training refs cannot fill a batch of {batch}: raise --images")
    if kind == "hbm":
        torch.cuda.synchronize()
        t0 = time.time()
        cache = HbmReferCache(ds, size)      # (synchronises before it returns)
        return HbmLoader(cache, batch_size=batch, shuffle=True, drop_last=True), time.time() - t0, cache.nbytes()
    return DataLoader(ds, batch_size=batch, num_workers=2, pin_memory=True, shuffle=True, drop_last=True,
                      persistent_workers=True), 0.0, 0


def _fed_steps(loader, n, step):
    """n steps of train_one_epoch's loop body over as many epochs as it takes; -> the last step's losses"""
    done, last = 0, None
    while done < n:
        for samples, targets in loader:
            word_ids = samples["word_ids"].squeeze(1).cuda(non_blocking=True)
            img = samples["img"].cuda(non_blocking=True)
            pseudo = targets["pseudo_gt"].cuda(non_blocking=True)
            last = step(img, word_ids, pseudo)
            done += 1
            if done == n:
                break
    return last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 20; 300 when fed by a loader)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--loader", choices=["synthetic", "dataloader", "hbm"], default="synthetic")
    ap.add_argument("--arith", default="h2,x3", help="arithmetics of the dense products to run, comma separated")
    ap.add_argument("--model_ema", action="store_true", help="EMA consistency training (the teacher forward, l5, the update)")
    ap.add_argument("--images", type=int, default=192, help="images of the synthetic dataset on disk (loader legs; >= 96)")
    a = ap.parse_args()
    if a.steps is None:
        a.steps = 20 if a.loader == "synthetic" else 300
    import warnings
    from tris_amd import ops
    from tris_amd.args import get_parser
    from tris_amd.model.model_stage2 import TRIS
    from tris_amd.optim import FusedAdamW
    from tris_amd.train_stage2 import train_step
    from tris_amd.utils.synth import seed_fill, synthetic_batch
    args = get_parser().parse_args(["--backbone", "clip-RN50", "--size", "320", "--max_query_len", "20"])
    b = synthetic_batch(a.batch, 320, 20, 0, seed=7)
    img, ids = b["img"].cuda(), b["word_ids"].cuda()
    tgt = torch.randint(0, 3, (a.batch, 1, 320, 320), generator=torch.Generator().manual_seed(3)).cuda()
    loader, build_s, cache_bytes, tmp = None, None, None, None
    if a.loader != "synthetic":
        from tris_amd.utils.synth import make_mini_refer, make_pseudo_masks
        tmp = tempfile.TemporaryDirectory(prefix="stage2_bench_")
        root = make_mini_refer(tmp.name, n_images=max(a.images, 96), seed=0, sizes=[(480, 640), (427, 640), (640, 480)])
        make_pseudo_masks(root, os.path.join(root, "pseudo"))
        loader, build_s, cache_bytes = _fed_loader(a.loader, root, a.batch)
    for mode in a.arith.split(","):
        ops.set_gemm_mode(mode)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = TRIS(args).cuda()
        seed_fill(model.state_dict(), 1234)
        ema = None
        if a.model_ema:       # built where train_stage2.main builds it: before model.train() (its trunk stays in eval mode)
            from tris_amd.ema import EMA
            ema = EMA(model)
        model.train()
        bb, hd = model.trainable_parameters()
        opt = FusedAdamW([{"params": bb, "lr": args.lr * args.lr_multi}, {"params": hd, "lr": args.lr}], lr=args.lr,
                         weight_decay=args.weight_decay)
        if ema is not None:
            ema.bind(opt)
        if loader is None:
            for _ in range(a.warmup):
                train_step(model, opt, img, ids, tgt, ema, ema is not None)
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(a.steps):
                last = train_step(model, opt, img, ids, tgt, ema, ema is not None)
        else:
            def step(*batch):
                return train_step(model, opt, *batch, ema, ema is not None)
            _fed_steps(loader, a.warmup, step)
            torch.cuda.synchronize()
            t0 = time.time()
            last = _fed_steps(loader, a.steps, step)
        torch.cuda.synchronize()
        dt = (time.time() - t0) / a.steps
        print(json.dumps({"metric": "stage2_train_img_per_s", "arith": mode, "value": round(a.batch / dt, 1),
                          "ms_per_step": round(1e3 * dt, 2), "batch": a.batch, "size": 320, "steps": a.steps,
                          "loss": float(last[0]), "model_ema": ema is not None, "l5": float(last[5]) if ema is not None else 0.0,
                          "assumed_gflop_per_img_fwd_on_top_of_trunk_text": DECODER_GFLOP + PIXATTN_GFLOP,
                          "loader": a.loader, "cache_build_s": None if build_s is None else round(build_s, 3),
                          "cache_bytes": cache_bytes}),
              flush=True)
        del model, opt, ema
        torch.cuda.empty_cache()
    del loader      # (ends the DataLoader's workers before the dataset directory goes)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
