"""Times the IRNet edge / displacement network (tris_amd/irn_net.py, csrc/irnnet.hip) on the GPU at image sizes 640x480, 480x640
and 320x320 (W x H), in both arithmetics of the dense products.

    python tools/irn_net_bench.py [--out profiles/irn_net_bench.jsonl] [--reps 7] [--inner 10] [--modes h2,x3] [--once WxH]

Per (size, arithmetic) one JSON line: milliseconds per image (one B = 2 pass: the image and its flip) for the whole network, split
into stem + pool, trunk, edge branch, displacement branch (each timed on the stage's own inputs), and make_ins_seg end to end:
the network plus the post-network synthesis (tris_amd/irn.py) on the network's (edge, dp) and a synthetic response map -- with
the seeded weights dp is noise, so the synthesis sees a scene of its own kind; its share is reported, not compared.
Weights: utils.synth.irn_fill.  A timed window is `inner` back-to-back calls between two device synchronises on a host clock,
after a warm-up; the median of `reps` windows divided by `inner` is reported.

--once WxH: one warmed-up pass at that size and nothing else (the target of a kernel-trace profile).
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

SIZES = [(480, 640), (640, 480), (320, 320)]      # (H, W)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=7, type=int)
    ap.add_argument("--inner", default=10, type=int)
    ap.add_argument("--modes", default="h2,x3")
    ap.add_argument("--once", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "irn_net_bench needs the MI355X"
    from tris_amd import irn, ops
    from tris_amd.irn_net import EdgeDisplacement
    from tris_amd.utils.synth import irn_fill, irn_image
    net = EdgeDisplacement()
    irn_fill(net.state_dict(), 0, 1.0)
    net.cuda()
    if args.once:
        W, H = (int(v) for v in args.once.split("x"))
        img = torch.from_numpy(irn_image(H, W, seed=1)).cuda()
        for mode in args.modes.split(","):
            ops.set_gemm_mode(mode)
            for _ in range(3):
                net(img)
        torch.cuda.synchronize()
        return
    rows = []
    for mode in args.modes.split(","):
        ops.set_gemm_mode(mode)
        for H, W in SIZES:
            img = torch.from_numpy(irn_image(H, W, seed=1)).cuda()
            rng = np.random.RandomState(0)
            low = rng.rand((H - 1) // 4 + 1, (W - 1) // 4 + 1).astype(np.float32)
            cam = torch.from_numpy(np.repeat(np.repeat(low, 4, 0), 4, 1)[:H, :W].copy()).cuda()
            r = {"image": f"{W}x{H}", "arith": mode}
            with torch.no_grad(), ops.autotune_off():
                out = net.forward_raw(img, taps=True)
                net._prepare(img.device)
                x1, taps = out["taps"][0], out["taps"]
                r["stem_pool_ms"] = timed(lambda: net._stem(img), args.reps, args.inner)
                r["trunk_ms"] = timed(lambda: net._trunk(x1), args.reps, args.inner)
                r["edge_branch_ms"] = timed(lambda: net.heads(taps, only="edge"), args.reps, args.inner)
                r["dp_branch_ms"] = timed(lambda: net.heads(taps, only="dp"), args.reps, args.inner)
            r["network_ms"] = timed(lambda: net(img), args.reps, args.inner)

            def end_to_end():
                edge, dp = net(img)
                return irn.make_ins_seg(cam, edge, dp, (H, W))
            res = end_to_end()
            r["instances_fragments"] = int(len(res["score"]))
            r["make_ins_seg_ms"] = timed(end_to_end, args.reps, max(args.inner // 2, 1))
            r["network_share"] = r["network_ms"] / r["make_ins_seg_ms"]
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(dict(r, device=torch.cuda.get_device_name(0), reps=args.reps, inner=args.inner)) + "\n")


if __name__ == "__main__":
    main()
