"""Times the target + scoring half of the ReferIt evaluation loop on the GPU, per image, on a synthetic set:

    python tools/referit_eval_bench.py [--out profiles/referit_eval_bench.jsonl] [--reps 7] [--inner 20]

* `grouped`: ops.rle_decode_sum_arena (run lengths resident in HBM) + ops.eval_post_group + the one fetch of the records --
  what tris_amd.validate_referit does per image behind the HBM cache.
* `parent`: what the tree offered before csrc/referit.hip -- per sentence cocomask.decode(rle).sum(2).astype(uint8) on the host
  (dataset/Dataset_referit.py:141-144), an upload, `!= 0`, ops.eval_post; one fetch of the K results.
* `decode_ms` / `score_ms`: the two kernels' calls alone (no fetch).

An image is K sentences of two overlapping blob-like segments each at H x W, scored from S x S response maps.  A timed window is
`inner` back-to-back images between two device synchronises on a host clock, after a warm-up of the same shapes; the median of
`reps` windows divided by `inner` is reported, in milliseconds per image.  Prints one JSON line per row.  The model's forward is
the same in both forms and is not part of the window.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [(360, 480, 3), (360, 480, 8), (480, 640, 5)]
LAUNCHES = {"grouped": 1 + 4, "parent_per_sentence": 3}


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def timed(fn, reps, inner, warmup=2):
    for _ in range(warmup):
        fn()
    return float(np.median([window(fn, inner) for _ in range(reps)]))


def blob_rles(H, W, seed):
    import oracle_boxes as OB
    import oracle_referit as O
    return [O.rle(OB.blob_mask(H, W, seed + j, q=0.8, sigma=6.0)) for j in range(2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=7, type=int)
    ap.add_argument("--inner", default=20, type=int)
    ap.add_argument("--size", default=320, type=int)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "referit_eval_bench needs the MI355X"
    from tris_amd import ops
    from tris_amd.dataset import cocomask
    from tris_amd.dataset.rle_arena import RleArena
    rows = []
    for H, W, K in CASES:
        sents = [blob_rles(H, W, 10 * k) for k in range(K)]
        arena = RleArena()
        ranges = torch.tensor([arena.add_sentence(s, H, W) for s in sents], dtype=torch.int32).cuda()
        ends, seg_off = arena.to("cuda")
        maps = torch.randn(K, 1, args.size, args.size, generator=torch.Generator().manual_seed(K)).relu().cuda()

        def decode():
            return ops.rle_decode_sum_arena(ends, seg_off, ranges, H, W)
        tg = decode()

        def score():
            return ops.eval_post_group(maps, tg, cams=None)

        def grouped():
            return ops.eval_post_group(maps, decode(), cams=None)[0].tolist()

        def parent():
            ius = []
            for k in range(K):
                t = torch.from_numpy(cocomask.decode(sents[k]).sum(axis=2).astype(np.uint8)).cuda()
                ius.append(ops.eval_post(maps[k], (t != 0).to(torch.uint8))[0])
            return torch.stack(ius).tolist()
        a, b = grouped(), parent()
        assert [r[:3] for r in a] == b, "the two forms disagree"
        r = {"size": f"{H}x{W}", "K": K, "map": args.size, "runs": int(ends.numel() - 1), "launches_grouped": LAUNCHES["grouped"],
             "launches_parent": LAUNCHES["parent_per_sentence"] * K}
        r["decode_ms"] = round(timed(decode, args.reps, args.inner), 4)
        r["score_ms"] = round(timed(score, args.reps, args.inner), 4)
        r["grouped_ms_per_image"] = round(timed(grouped, args.reps, args.inner), 4)
        r["parent_ms_per_image"] = round(timed(parent, args.reps, max(args.inner // 4, 1)), 4)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps({"device": torch.cuda.get_device_name(0), "tool": "tools/referit_eval_bench.py", "reps": args.reps,
                                    "inner": args.inner, **r}) + "\n")


if __name__ == "__main__":
    main()
