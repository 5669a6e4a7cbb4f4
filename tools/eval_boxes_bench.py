"""Times the box-metric pass of `validate` (ops.eval_boxes, csrc/boxes.hip) on the GPU, per (image, sentence):

    python tools/eval_boxes_bench.py [--out profiles/eval_boxes_bench.jsonl] [--reps 7] [--inner 20] [--throughput]

* ops.eval_post alone and ops.eval_post + ops.eval_boxes on 320 x 320 response maps resized to 427 x 640 and 480 x 640, for a map
  with few proposals and one with a few hundred (a Gaussian-smoothed normal field minus its 0.7 quantile, clipped at zero; the
  smoothing width sets the number of blobs).  Each row reports the proposals / NMS survivors / kept boxes the mask really has.
* kernel launches per call, counted from the launch sequences of csrc/eval.hip and csrc/boxes.hip.
* with --throughput: refs/s of tools/eval_throughput.py with cfg.eval_boxes off and on (its seed-filled model answers with all-one
  masks, i.e. the pass's short path: labelling and scans, no proposals).

A timed window is `inner` back-to-back calls between two device synchronises on a host clock, after a warm-up of the same shapes;
the median of `reps` windows divided by `inner` is reported, in milliseconds per call.  Prints one JSON line per row.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("TRIS_RANDOM_INIT", "1")
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(427, 640), (480, 640)]
SIGMAS = [("few", 24.0), ("many", 2.5)]
LAUNCHES = {"eval_post": 3, "eval_boxes": 8}


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


def blob_map(S, sigma, seed, q=0.7):
    """relu-like response map [1,1,S,S]: smoothed normal field minus its q quantile, clipped at zero"""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(1, 1, S, S, generator=g, dtype=torch.float64)
    r = int(3 * sigma)
    k = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=torch.float64) / sigma) ** 2)
    k = k / k.sum()
    f = torch.nn.functional.conv2d(torch.nn.functional.pad(f, (r, r, 0, 0), mode="circular"), k.reshape(1, 1, 1, -1))
    f = torch.nn.functional.conv2d(torch.nn.functional.pad(f, (0, 0, r, r), mode="circular"), k.reshape(1, 1, -1, 1))
    return (f - f.flatten().quantile(q)).clamp(min=0).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=7, type=int)
    ap.add_argument("--inner", default=20, type=int)
    ap.add_argument("--throughput", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_boxes_bench needs the MI355X"
    from tris_amd import ops
    rows = []
    for H, W in SIZES:
        for tag, sigma in SIGMAS:
            m = blob_map(320, sigma, seed=11).cuda()
            tgt = torch.zeros(H, W, dtype=torch.uint8, device="cuda")
            tgt[H // 4:H // 2, W // 4:W // 2] = 1
            gt = ops.eval_boxes_gt([W // 4, H // 4, W // 2, H // 2])[0]

            def post():
                return ops.eval_post(m, tgt)

            def both():
                iu, cam = ops.eval_post(m, tgt)
                return ops.eval_boxes(cam, tgt, gt, iu)
            rec = ops.decode_boxes_record(both().tolist())
            r = {"size": f"{H}x{W}", "mask": tag, "proposals": rec["n_prop"], "nms_survivors": rec["n_nms"], "kept": rec["n_kept"],
                 "launches_eval_post": LAUNCHES["eval_post"], "launches_eval_boxes": LAUNCHES["eval_boxes"]}
            r["eval_post_ms"] = round(timed(post, args.reps, args.inner), 4)
            r["eval_post_plus_boxes_ms"] = round(timed(both, args.reps, args.inner), 4)
            r["eval_boxes_ms"] = round(r["eval_post_plus_boxes_ms"] - r["eval_post_ms"], 4)
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.throughput:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import eval_throughput
        from tris_amd.config import cfg
        import warnings
        from tris_amd.args import get_parser
        from tris_amd.model.model_stage1 import TRIS
        from tris_amd.utils.synth import seed_fill
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = TRIS(get_parser().parse_args(["--size", "320", "--max_query_len", "20"])).cuda()
        seed_fill(model.state_dict(), 1234)
        for on in (False, True, False, True):
            with cfg.override(eval_boxes=on):
                t = eval_throughput.measure(groups=(1, 16), model=model)
            r = {"eval_throughput": True, "eval_boxes": int(on), "by_group": t["by_group"]}
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, **r}) + "\n")


if __name__ == "__main__":
    main()
