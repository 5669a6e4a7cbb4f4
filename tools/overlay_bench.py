"""Times the heat-map overlay of single-image inference (ops.cam_paint, csrc/overlay.hip) on the GPU:

    python tools/overlay_bench.py [--out profiles/overlay_bench.jsonl] [--reps 7] [--inner 50]

* ops.cam_paint of K = 1 and K = 8 response maps (320 x 320) onto a 480 x 640 picture: two launches per call;
* the same figure composed from what the library had before: ops.resize_bilinear (align_corners=True), torch reductions, the
  normalisation, the quantisation, an index into the colour table and the integer blend.  Its heat bytes are compared with
  cam_paint's before anything is timed (they may differ at a quantisation step only, a few pixels per million).

A timed window is `inner` back-to-back calls between two HIP events on the current stream, after a warm-up of the same shapes; the
median of `reps` windows divided by `inner` is reported in microseconds per call, with the bytes the pass must move (maps in, the
picture once per sentence, heat out) over that time against the 8 TB/s the other sections use.  One JSON line per row.
"""
import argparse
import json
import os
import sys

os.environ.setdefault("TRIS_RANDOM_INIT", "1")
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, S = 480, 640, 320
HBM_TBS = 8.0


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def timed(fn, reps, inner, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([window(fn, inner) for _ in range(reps)]))


def composed(ops, maps, image, lut):
    """the presentation pass from the library's resize and torch ops"""
    K = maps.shape[0]
    u = ops.resize_bilinear(maps.reshape(K, 1, S, S), (H, W), True).reshape(K, -1).clamp_(min=0)
    lo, hi = u.amin(1, keepdim=True), u.amax(1, keepdim=True)
    idx = ((u - lo) / (hi - lo + 1e-5) * 255).to(torch.int64).clamp_(0, 255)
    col = lut.to(torch.int32)[idx].reshape(K, H, W, 3)
    heat = ((3 * col + 2 * image.to(torch.int32) + 2) // 5).to(torch.uint8)
    return heat, torch.cat([lo, hi], 1), u.argmax(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=7, type=int)
    ap.add_argument("--inner", default=50, type=int)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "overlay_bench needs the MI355X"
    from tris_amd import ops
    from tris_amd.predict import JET
    lut = torch.from_numpy(JET.copy()).cuda()
    image = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (H, W, 3)).astype(np.uint8)).cuda()
    rows = []
    for K in (1, 8):
        maps = torch.from_numpy(np.random.RandomState(2).uniform(-1, 1, (K, S, S)).astype(np.float32)).cuda()
        a, b = ops.cam_paint(maps, image, lut), composed(ops, maps, image, lut)
        differ = int((a[0] != b[0]).any(-1).sum())
        moved = K * (S * S * 4 + 2 * H * W * 3)                     # maps in, the picture once per sentence, heat out
        r = {"size": f"{H}x{W}", "source": f"{S}x{S}", "K": K, "bytes_moved": moved, "pixels_differing_from_composed": differ,
             "argmax_equal_to_composed": bool(torch.equal(a[3], b[2])), "launches_cam_paint": 2}
        r["cam_paint_us"] = round(timed(lambda: ops.cam_paint(maps, image, lut), args.reps, args.inner), 2)
        r["composed_us"] = round(timed(lambda: composed(ops, maps, image, lut), args.reps, args.inner), 2)
        r["cam_paint_fraction_of_8TBs"] = round(moved / (r["cam_paint_us"] * 1e-6) / (HBM_TBS * 1e12), 4)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, **r}) + "\n")


if __name__ == "__main__":
    main()
