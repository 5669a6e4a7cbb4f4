"""Stage-2 training throughput on one MI355X: img/s and ms/step of eager train_stage2.train_step at B = 48, 320 px, T = 20, in
both arithmetics of the dense products (h2, x3).  Seed-filled weights, synthetic images / tokens / pseudo targets.

    python tools/stage2_bench.py [--steps 20] [--warmup 5] [--batch 48]

Prints one JSON line per arithmetic.  No target is set; the FLOP count it assumes is printed with it (forward, per image:
the trunk + text encoder of Stage-1 plus the decoder and the three PixelAttentions, computed from the shapes)."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("TRIS_RANDOM_INIT", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

DECODER_GFLOP = 9.2      # the twelve 3x3 convolutions + heads, per image forward at 320 px (computed from the shapes)
PIXATTN_GFLOP = 10.1     # attention2..4 at 40^2 / 20^2 / 10^2, T = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=48)
    a = ap.parse_args()
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
    for mode in ("h2", "x3"):
        ops.set_gemm_mode(mode)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = TRIS(args).cuda().train()
        seed_fill(model.state_dict(), 1234)
        bb, hd = model.trainable_parameters()
        opt = FusedAdamW([{"params": bb, "lr": args.lr * args.lr_multi}, {"params": hd, "lr": args.lr}], lr=args.lr,
                         weight_decay=args.weight_decay)
        for _ in range(a.warmup):
            train_step(model, opt, img, ids, tgt)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(a.steps):
            last = train_step(model, opt, img, ids, tgt)
        torch.cuda.synchronize()
        dt = (time.time() - t0) / a.steps
        print(json.dumps({"metric": "stage2_train_img_per_s", "arith": mode, "value": round(a.batch / dt, 1),
                          "ms_per_step": round(1e3 * dt, 2), "batch": a.batch, "size": 320, "steps": a.steps,
                          "loss": float(last[0]), "assumed_gflop_per_img_fwd_on_top_of_trunk_text": DECODER_GFLOP + PIXATTN_GFLOP}),
              flush=True)
        del model, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
