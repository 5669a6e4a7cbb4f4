"""Times the build of HbmReferCache with cfg.poly_targets off and on, on the GPU, and records what the cache then holds:

    python tools/poly_targets_bench.py [--out profiles/poly_targets_bench.jsonl] [--images 150] [--vertices 60] [--size 320] [--reps 3]

* The split is synthetic (tris_amd.utils.synth.make_mini_refer) at COCO-like image sizes, a few hundred refs; every polygon is
  resampled to `--vertices` vertices along its outline with a small radial jitter (RefCOCO outlines have tens of vertices, the
  generator's have 3-7), and every fifth annotation gets a second, overlapping polygon.
* A first cache (knob off) is built once as warm-up and as the donor of the decoded images (`images_from=`), so that the timed
  builds hold what the knob changes: the targets (and the token rows, the same under both values).  One full build per value,
  images included, is timed too.
* Rows: training and evaluation cache of the same refs, knob 0 and 1 alternating, the median of `--reps` builds between two device
  synchronises on a host clock; `nbytes` is HbmReferCache.nbytes() of the last build (images shared with the donor not counted).
* The knob-off build of the same run on the same box is the baseline.  Nothing asserts on the times; the batches of the two caches
  are compared by tests/test_gpu_poly.py.

Appends one JSON line per row to --out and prints it.
"""
import argparse
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("TRIS_RANDOM_INIT", "1")
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(480, 640), (427, 640), (640, 480), (375, 500), (640, 427), (500, 333)]


def densify(root, vertices, seed=0):
    """instances.json rewritten in place -> number of polygons"""
    rng = np.random.RandomState(seed)
    path = os.path.join(root, "refer", "refcocog", "instances.json")
    inst = json.load(open(path))
    n = 0
    for k, a in enumerate(inst["annotations"]):
        p = np.asarray(a["segmentation"][0], np.float64).reshape(-1, 2)
        closed = np.concatenate([p, p[:1]])
        seg = np.concatenate([[0.0], np.cumsum(np.hypot(*np.diff(closed, axis=0).T))])
        t = np.linspace(0.0, seg[-1], vertices, endpoint=False)
        q = np.stack([np.interp(t, seg, closed[:, 0]), np.interp(t, seg, closed[:, 1])], 1)
        c = q.mean(0)
        q = c + (q - c) * rng.uniform(0.9, 1.1, (vertices, 1))
        polys = [q]
        if k % 5 == 0:
            polys.append(q + [0.3 * (q[:, 0].max() - q[:, 0].min()), 2.0])
        a["segmentation"] = [x.round(2).reshape(-1).tolist() for x in polys]
        n += len(polys)
    json.dump(inst, open(path, "w"))
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", default=150, type=int)
    ap.add_argument("--vertices", default=60, type=int)
    ap.add_argument("--size", default=320, type=int)
    ap.add_argument("--reps", default=3, type=int)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "poly_targets_bench needs the MI355X"
    from tris_amd.config import cfg
    from tris_amd.dataset.ReferDataset import ReferDataset
    from tris_amd.dataset.hbm import HbmReferCache
    from tris_amd.dataset.transform import get_transform
    from tris_amd.utils.synth import make_mini_refer, word_hash_tokenize
    S = args.size
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        root = make_mini_refer(tmp, n_images=args.images, seed=3, sizes=SIZES)
        n_poly = densify(root, args.vertices)

        def dataset(eval_mode):
            return ReferDataset(refer_data_root=root, dataset="refcocog", splitBy="umd", max_tokens=20, split="train", size=S,
                                image_transforms=get_transform(S, not eval_mode), eval_mode=eval_mode, tokenizer=word_hash_tokenize)

        def build(ds, knob, donor):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with cfg.override(poly_targets=bool(knob)):
                c = HbmReferCache(ds, S, images_from=donor)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, c
        sets = {"train": dataset(False), "eval": dataset(True)}
        donor = build(sets["train"], 0, None)[1]
        build(sets["train"], 1, donor)                      # (warm-up of the knob-on launches and index tables)
        common = {"device": torch.cuda.get_device_name(0), "refs": len(sets["train"]), "polygons_in_file": n_poly, "images": args.images,
                  "vertices": args.vertices, "size": S, "reps": args.reps}
        for mode, ds in sets.items():
            times, nbytes = {0: [], 1: []}, {}
            for _ in range(args.reps):
                for knob in (0, 1):
                    t, c = build(ds, knob, donor)
                    times[knob].append(t)
                    nbytes[knob] = c.nbytes()
                    del c
            for knob in (0, 1):
                rows.append({**common, "cache": mode, "poly_targets": knob, "images_shared": True,
                             "build_s": round(float(np.median(times[knob])), 4), "build_s_all": [round(t, 4) for t in times[knob]],
                             "nbytes": int(nbytes[knob])})
                print(json.dumps(rows[-1]), flush=True)
        del donor
        for knob in (0, 1):
            t, c = build(sets["eval"], knob, None)
            rows.append({**common, "cache": "eval", "poly_targets": knob, "images_shared": False, "build_s": round(t, 4),
                         "build_s_all": [round(t, 4)], "nbytes": int(c.nbytes())})
            print(json.dumps(rows[-1]), flush=True)
            del c
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
