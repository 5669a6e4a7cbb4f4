"""Times the scoring of response maps against REFER ground truth (ops.score_maps, csrc/labelscore.hip):

    python tools/pseudo_eval_bench.py [--out profiles/pseudo_eval_bench.jsonl] [--reps 7] [--inner 20] [--limit 300]

Shape: one group of 8 response maps of 480 x 640 (the names of one image), the default sweep of 20 thresholds, 8 refs of one polygon
each (a 14-vertex blob, a few hundred runs).  Four routes to the same I and U of every (name, threshold), microseconds per name:
* score_maps -- ops.score_maps on run ends as pseudo_eval calls it: argument checks, the upload of the 8 ranges, two launches;
* launches   -- the same two launches through the C ABI with everything already on the device: what the device spends;
* device     -- a restatement from ops that were here before: ops.rle_decode_sum_arena to a full-size target, then per threshold
                torch comparisons and sums on the device;
* host       -- cocomask.frPyObjects + decode of every ref and numpy comparisons per threshold (one pass, wall clock).
Every route is compared with the host route before it is timed.

A fifth route, score_planes (ops.score_planes), has a shape of its own: K = 4 instance masks of 480 x 640 against one of the refs.
It is timed beside the composition that gave the same [K+3, 2] table before the op existed -- K + 1 calls of ops.score_counts, the
stack and each plane alone -- with the two alternated window by window in one process (windows of 100 x `inner` calls), and alone on the 320 x 320 NEAREST grid
(which the composition cannot score).  Both are compared with a numpy count over the host-rasterised ref first.  Its line carries the
median and the lowest and highest window of each.

A timed window is `inner` back-to-back calls between two HIP events on the current stream, after a warm-up; the median of `reps`
windows divided by `inner` and by the 8 names is reported.  Every route runs in a child process of its own under a time limit of
`limit` seconds, and nothing more is started after one that fails.  One JSON line per route.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

G, H, W = 8, 480, 640
ROUTES = ("score_maps", "launches", "device", "host", "score_planes")
K_PLANES, TRAIN_SIZE = 4, 320


def scene():
    """-> (maps float32 [G,H,W], polygons: one per ref, thresholds)"""
    import numpy as np
    from tris_amd.pseudo_eval import default_thresholds
    rng = np.random.RandomState(17)
    polys, maps = [], np.empty((G, H, W), np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    for g in range(G):
        cx, cy, r = rng.uniform(0.3, 0.7) * W, rng.uniform(0.3, 0.7) * H, rng.uniform(90, 130)
        ang = np.sort(rng.uniform(0, 2 * np.pi, 14))
        rad = r * rng.uniform(0.7, 1.0, 14)
        polys.append(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).round(2).reshape(-1).tolist())
        bump = np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * (0.8 * r) ** 2))
        maps[g] = np.maximum(bump + 0.15 * rng.randn(H, W), 0)            # a ReLU'd map: a share of exact zeros
        maps[g] /= maps[g].max()
    return maps, polys, default_thresholds()


def window(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def timed(fn, reps, inner, warmup=3):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([window(fn, inner) for _ in range(reps)]))


def host_iu(maps, polys, thr):
    import numpy as np
    from tris_amd.dataset import cocomask
    t32 = np.asarray(thr, np.float32)
    I, U = np.zeros((G, t32.size), np.int64), np.zeros((G, t32.size), np.int64)
    for g in range(G):
        gt = cocomask.decode(cocomask.frPyObjects([polys[g]], H, W)).sum(2) == 1
        for j, t in enumerate(t32):
            pred = maps[g] > t
            I[g, j], U[g, j] = np.count_nonzero(pred & gt), np.count_nonzero(pred | gt)
    return I, U


def planes_scene(polys):
    """-> (stack uint8 [K,H,W]: discs around the first ref's polygon and one fragment, ground truth bool [H,W] of that ref)"""
    import numpy as np
    from tris_amd.dataset import cocomask
    gt = cocomask.decode(cocomask.frPyObjects([polys[0]], H, W)).sum(2) == 1
    xy = np.asarray(polys[0]).reshape(-1, 2)
    cx, cy = xy.mean(0)
    ys, xs = np.mgrid[0:H, 0:W]
    stack = np.zeros((K_PLANES, H, W), np.uint8)
    for k, (dx, dy, r) in enumerate([(0, 0, 95), (40, -30, 70), (-120, 60, 50), (200, 150, 6)][:K_PLANES]):
        stack[k] = (xs - cx - dx) ** 2 + (ys - cy - dy) ** 2 < r * r
    return stack, gt


def host_table(stack, gt, yi=None, xi=None):
    """the [K+3, 2] table by numpy counting, on the samples (yi[y], xi[x]) when given (Pillow's NEAREST tables have no hole here)"""
    import numpy as np
    if yi is not None:
        stack, gt = stack[:, yi[:, None], xi[None, :]], gt[yi[:, None], xi[None, :]]
    s = stack.astype(np.int64).sum(0)
    sels = [s == 0, s == 1, s >= 2] + [p != 0 for p in stack]
    return np.array([[np.count_nonzero(sel & ~gt), np.count_nonzero(sel & gt)] for sel in sels], np.int64)


def planes_route(reps, inner):
    import numpy as np
    import torch
    from tris_amd import ops
    from tris_amd.dataset import pil_tables
    from tris_amd.dataset.poly_arena import PolyArena
    _, polys, _ = scene()
    stack, gt = planes_scene(polys)
    arena = PolyArena()
    lo, hi = arena.add_ref([polys[0]], H, W, "ref 0")
    built = arena.build("cuda")
    dev = torch.from_numpy(stack).cuda()
    planes = [dev[k:k + 1].contiguous() for k in range(K_PLANES)]

    def new():
        return ops.score_planes(dev, built, lo, hi, H, W)

    def new_train():
        return ops.score_planes(dev, built, lo, hi, H, W, out_hw=TRAIN_SIZE)

    def composed():
        hist = ops.score_counts(dev, built, lo, hi, H, W)
        rows = [hist[0], hist[1], hist[2:].sum(0)]
        for p in planes:
            rows.append(ops.score_counts(p, built, lo, hi, H, W)[1:].sum(0))
        return torch.stack(rows)

    want = host_table(stack, gt)
    yi, xi = pil_tables.nearest_index(H, TRAIN_SIZE), pil_tables.nearest_index(W, TRAIN_SIZE)
    assert yi.min() >= 0 and xi.min() >= 0
    assert np.array_equal(new().cpu().numpy(), want), "score_planes disagrees with the host count"
    assert np.array_equal(composed().cpu().numpy(), want), "the score_counts composition disagrees with the host count"
    assert np.array_equal(new_train().cpu().numpy(), host_table(stack, gt, yi, xi)), "score_planes at 320 disagrees with the host count"
    for fn in (new, composed, new_train):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    inner *= 100                                                    # a call is some 10 us: windows of thousands of calls, not of 20
    w = {"planes": [], "composed": [], "planes_320": []}
    for _ in range(reps):                                           # alternated: one window of each, reps times
        w["planes"].append(window(new, inner))
        w["composed"].append(window(composed, inner))
        w["planes_320"].append(window(new_train, inner))
    row = {"route": "score_planes", "K": K_PLANES, "H": H, "W": W, "runs": int(built.seg_off[hi] - built.seg_off[lo]),
           "clock": "device events, routes alternated window by window in one process"}
    for key, v in w.items():
        row[f"{key}_us_per_name"] = round(float(np.median(v)), 3)
        row[f"{key}_us_low_high"] = [round(float(min(v)), 3), round(float(max(v)), 3)]
    row.update(train_size=TRAIN_SIZE, device=torch.cuda.get_device_name(0), reps=reps, inner=inner)
    print(json.dumps(row), flush=True)


def route(name, reps, inner):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "pseudo_eval_bench needs the MI355X"
    if name == "score_planes":
        return planes_route(reps, inner)
    from tris_amd import ops, pseudo_eval as pe
    from tris_amd.dataset.poly_arena import PolyArena
    maps, polys, thr = scene()
    want_I, want_U = host_iu(maps, polys, thr)
    arena = PolyArena()
    ranges = [arena.add_ref([p], H, W, f"ref {g}") for g, p in enumerate(polys)]
    built = arena.build("cuda")
    runs = np.diff(built.seg_off.cpu().numpy()).tolist()
    dev = torch.from_numpy(maps).cuda()
    checked = ops.ScoreThresholds(thr)
    t_dev = checked.dev(dev.device)
    row = {"route": name, "G": G, "H": H, "W": W, "T": len(thr), "runs_per_ref": [int(min(runs)), int(max(runs))]}

    def new():
        return ops.score_maps(dev, built, ranges, checked)

    def restated():
        gt = ops.rle_decode_sum_arena(built.ends, built.seg_off, built.ranges, H, W) == 1
        I, U = [], []
        for j in range(len(thr)):
            pred = dev > t_dev[j]
            I.append((pred & gt).sum((1, 2)))
            U.append((pred | gt).sum((1, 2)))
        return torch.stack(I, 1), torch.stack(U, 1)

    if name == "score_maps":
        I, U = pe.sweep_iu(new().cpu().numpy())
        assert np.array_equal(I, want_I) and np.array_equal(U, want_U), "score_maps disagrees with the host route"
        row["us_per_name"] = round(timed(new, reps, inner) / G, 3)
    elif name == "launches":
        from tris_amd import _lib
        hist = torch.empty(G, len(thr) + 1, 2, dtype=torch.int64, device="cuda")
        ws = ops.workspace(_lib.query("tris_score_workspace_bytes", G, H, W, len(thr) + 1))
        ptrs = [t.data_ptr() for t in (dev, built.ends, built.seg_off, built.ranges)]
        stream = torch.cuda.current_stream().cuda_stream

        def launches():
            _lib.call("tris_score_maps_f32", *ptrs, G, H, W, t_dev.data_ptr(), len(thr), 0, hist.data_ptr(), ws.data_ptr(), stream)
        launches()
        I, U = pe.sweep_iu(hist.cpu().numpy())
        assert np.array_equal(I, want_I) and np.array_equal(U, want_U), "the launches disagree with the host route"
        row["us_per_name"] = round(timed(launches, reps, inner) / G, 3)
    elif name == "device":
        I, U = restated()
        assert np.array_equal(I.cpu().numpy(), want_I) and np.array_equal(U.cpu().numpy(), want_U), "the restatement disagrees"
        row["us_per_name"] = round(timed(restated, reps, inner) / G, 3)
    else:
        t0 = time.perf_counter()
        host_iu(maps, polys, thr)
        row["us_per_name"] = round((time.perf_counter() - t0) * 1e6 / G, 1)
        row["clock"] = "wall, one pass"
    row.update(device=torch.cuda.get_device_name(0), reps=reps, inner=inner)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=7, type=int)
    ap.add_argument("--inner", default=20, type=int)
    ap.add_argument("--limit", default=300, type=int, help="seconds each route's process may take")
    ap.add_argument("--route", default=None, choices=ROUTES, help="(internal) run one route in this process")
    args = ap.parse_args()
    if args.route is not None:
        return route(args.route, args.reps, args.inner)
    rows = []
    for name in ROUTES:
        cmd = [sys.executable, os.path.abspath(__file__), "--route", name, "--reps", str(args.reps), "--inner", str(args.inner)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.limit)     # (TimeoutExpired ends the tool)
        if run.returncode != 0:
            raise SystemExit(f"route {name} ended with status {run.returncode}; nothing more is started\n{run.stdout[-2000:]}{run.stderr[-4000:]}")
        line = run.stdout.strip().splitlines()[-1]
        rows.append(json.loads(line))
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
