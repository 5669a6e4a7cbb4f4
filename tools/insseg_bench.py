"""Times the instance-mask synthesis (tris_amd/irn.py, csrc/insseg.hip) on the GPU at map sizes 80x80, 160x120 and 160x160.

    python tools/insseg_bench.py [--out results.json] [--reps 7] [--inner 20]

* the walk (256 steps) on exactly K in {1, 4, 16} instance rows, built independently of the scene (sparse random rows), and at
  80x80 the reference's own formulation on the same rows and the same GPU: the dense N x N transition matrix squared exp_times = 8
  times, then x @ T, with the project's ops.matmul (indexing.py:132-139; N = 6400, 164 MB per matrix; its assembly is not timed).
  The two are timed alternately, window by window.
* the other stages and make_ins_seg as a whole on a synthetic scene with K - 1 blobs (utils.synth.make_ins_seg_scene).  Blobs may
  overlap, so the row reports the number of instance rows and fragments the scene really has.

A timed window is `inner` back-to-back calls between two device synchronises on a host clock, after a warm-up of the same shapes;
the median of `reps` windows divided by `inner` is reported, in milliseconds per call.  make_ins_seg and the fragment stage include
their host side (small device-to-host reads and the copy of the result to numpy).  Prints one JSON line per row.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(80, 80), (160, 120), (160, 160)]
KS = [1, 4, 16]


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


def dense_transition(Wt, colsum, dirs):
    """the reference's matrix: dense symmetric affinity with unit diagonal, column-normalised (assembled with torch: not timed)"""
    nd, h, w = Wt.shape
    n = h * w
    A = torch.eye(n, device="cuda")
    idx = torch.arange(n, device="cuda")
    yy, xx = idx // w, idx % w
    for d in range(nd):
        dy, dx = int(dirs[d, 0]), int(dirs[d, 1])
        ok = (yy + dy < h) & (xx + dx >= 0) & (xx + dx < w)
        i, j = idx[ok], idx[ok] + dy * w + dx
        A[i, j] = Wt[d].reshape(-1)[ok]
        A[j, i] = Wt[d].reshape(-1)[ok]
    return A / colsum.reshape(1, n)


def dense_walk(v0, T, exp_times):
    from tris_amd import ops
    for _ in range(exp_times):
        T = ops.matmul(T, T)
    return ops.matmul(v0, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=7, type=int)
    ap.add_argument("--inner", default=20, type=int)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "insseg_bench needs the MI355X"
    from tris_amd import irn, ops
    from tris_amd.utils.synth import make_ins_seg_scene
    reps, inner = args.reps, args.inner
    rows = []
    with torch.no_grad():
        for h, w in SIZES:
            H, W = 4 * h - 2, 4 * w - 1
            for K in KS:
                cam, edge, dp = make_ins_seg_scene(H, W, n_blobs=K - 1, seed=K)
                cam_t, edge_t, dp_t = (torch.from_numpy(a).cuda() for a in (cam, edge, dp))
                dirs, off, cells = irn.device_tables(edge_t.device)
                Wt, colsum = ops.irn_affinity(edge_t, dirs, off, cells, 10)
                r = {"map": f"{h}x{w}", "image": f"{H}x{W}", "K": K}
                # the walk on exactly K rows
                gen = torch.Generator(device="cuda").manual_seed(K)
                xk = torch.rand(K, h, w, device="cuda", generator=gen) * (torch.rand(K, h, w, device="cuda", generator=gen) < 0.3)
                walk = lambda: ops.irn_walk(xk, edge_t, Wt, colsum, dirs, 256)   # noqa: E731
                if (h, w) == (80, 80):
                    T = dense_transition(Wt, colsum, dirs)
                    v0 = (xk * (1 - edge_t)).reshape(K, h * w)
                    dense = lambda: dense_walk(v0, T, 8)                          # noqa: E731
                    got, ref = walk(), dense().reshape(K, h, w)
                    r["dense_vs_sparse_max_rel_diff"] = float((ref - got).abs().max() / got.abs().max())
                    walk(), dense()
                    tw, td = [], []
                    for _ in range(reps):                                         # alternating windows
                        tw.append(window(walk, inner))
                        td.append(window(dense, max(inner // 4, 1)))
                    r["walk_ms"], r["dense_8_squarings_ms"] = float(np.median(tw)), float(np.median(td))
                    del T, ref
                    torch.cuda.empty_cache()
                else:
                    r["walk_ms"] = timed(walk, reps, inner)
                # the other stages on the scene's own intermediates
                cen = ops.irn_centroids(dp_t)
                inst, k = irn._instance_map(cen, dp_t)
                x = ops.irn_instance_cam(ops.resize_bilinear(cam_t[None, None], (h, w), True)[0, 0], inst, k)
                rw = ops.irn_walk(x, edge_t, Wt, colsum, dirs, 256)
                up, labels = ops.irn_finish(rw, (H, W), 0.25)
                out = irn.make_ins_seg(cam, edge, dp, (H, W))
                r["scene_blobs"], r["scene_K"], r["scene_fragments"] = K - 1, k, int(len(out["score"]))
                r["centroids_ms"] = timed(lambda: ops.irn_centroids(dp_t), reps, inner)
                r["instance_map_ms"] = timed(lambda: irn._instance_map(cen, dp_t), reps, inner)
                r["affinity_ms"] = timed(lambda: ops.irn_affinity(edge_t, dirs, off, cells, 10), reps, inner)
                r["scene_walk_ms"] = timed(lambda: ops.irn_walk(x, edge_t, Wt, colsum, dirs, 256), reps, inner)
                r["finish_ms"] = timed(lambda: ops.irn_finish(rw, (H, W), 0.25), reps, inner)
                r["fragments_ms"] = timed(lambda: irn._fragments(up, labels, k, np.zeros(k, np.int64), H * W * 0.01), reps, inner)
                r["make_ins_seg_ms"] = timed(lambda: irn.make_ins_seg(cam, edge, dp, (H, W)), reps, inner)
                rows.append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "inner": inner, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
