"""Records tests/golden/g14_insseg.npz from the REAL reference functions of IRNet's instance-mask synthesis
(IRNet/step_refer/make_ins_seg_labels.py, IRNet/misc/indexing.py), imported through stubs of the packages this stack does not
have.  Build-machine tool: the reference tree is not on the GPU machines, and nothing that runs there reads it.

    python tools/gen_golden_insseg.py

Stubs: skimage.measure.label -> scipy.ndimage.label with the 4-neighbour structure (components numbered by first pixel in raster
order, as skimage does), cv2 / pydensecrf / voc12.dataloader -> empty modules (imported, never called), Tensor.cuda -> identity.

Per scene s (synthetic, at most 22 x 44 maps, image sizes (4h-2, 4w-1)): the inputs cam / edge / dp / size, every intermediate
(centroids, instance map, instance cams, rw, rw_up, label map) and the final dict, all from the reference's functions; the tensor
operations its worker does between them (resize, x4 upsample, normalise, arg-max against a constant background plane) are
written here with torch.  Plus PathIndex.search_paths.
The generator asserts what the tests rely on, and moves to the next seed otherwise: >= 2 scenes with >= 3 instances, a fragment
below 1 % of the image in >= 1 scene, an instance that splits into several fragments in >= 1 scene, and at most 0.5 % of the pixels of any scene with a top-1 / top-2 gap below 1e-3.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g14_insseg.npz")

# (h, w, number of blobs)
SCENES = [(20, 30, 2), (22, 44, 3), (20, 20, 1)]
BETA, EXP_TIMES, BG_THRES = 10, 8, 0.25


def reference_modules():
    from oracle.ref_shim import REF_ROOT
    import scipy.ndimage

    def label(img, connectivity=1, background=0):
        assert connectivity == 1 and background == 0
        return scipy.ndimage.label(np.asarray(img) != 0, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])[0]

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    measure = stub("skimage.measure", label=label)
    stub("skimage", measure=measure)
    stub("cv2")
    stub("pydensecrf.densecrf")
    stub("pydensecrf.utils", unary_from_labels=None)
    stub("pydensecrf")
    stub("voc12.dataloader")
    stub("voc12")
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(REF_ROOT, "IRNet"))
    from misc import indexing, pyutils                    # noqa: E402  (the reference's)
    from step_refer import make_ins_seg_labels as labels  # noqa: E402
    return indexing, pyutils, labels


def make_scene(h, w, n_blobs, rng):
    """blobs whose displacement field points to their centre with strength 0.8 * distance (> 2.5 off the centre, so each centre
    is a weak region of its own), an edge ring on every rim, two walled pockets in the background and a response map that is
    high inside the blobs and the pockets"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    dp = np.zeros((2, h, w), np.float32)
    edge = (0.05 + 0.1 * rng.random((h, w))).astype(np.float32)
    lowres = (0.02 + 0.03 * rng.random((h, w))).astype(np.float32)
    taken = np.zeros((h, w), bool)
    for _ in range(n_blobs):
        for _try in range(200):
            r = rng.uniform(5.0, 6.5)
            cy, cx = rng.uniform(r + 0.5, h - r - 1.5), rng.uniform(r + 0.5, w - r - 1.5)
            dist = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            if not taken[dist < r + 1.5].any():
                break
        else:
            raise RuntimeError("no room")
        inside = dist <= r
        taken |= dist < r + 1
        dp[0][inside] = ((cy - yy) * 0.8)[inside]
        dp[1][inside] = ((cx - xx) * 0.8)[inside]
        edge[np.abs(dist - r) < 0.8] = 0.9 + 0.08 * rng.random()
        lowres[dist < r - 1] = rng.uniform(0.5, 1.0) * (1 + 0.2 * rng.random((h, w)).astype(np.float32))[dist < r - 1]
    # two pockets of the background instance, each inside a one-cell wall, somewhere free: 2 x 3 cells (a fragment below 1 % of
    # the image) and 4 x 5 cells (above it), so that instance has two fragments, one of them scored 0
    for ph, pw in ((2, 3), (4, 5)):
        for _try in range(500):
            py, px = rng.integers(1, h - ph - 1), rng.integers(1, w - pw - 1)
            if not taken[py - 1:py + ph + 1, px - 1:px + pw + 1].any():
                edge[py - 1:py + ph + 1, px - 1:px + pw + 1] = 0.95
                edge[py:py + ph, px:px + pw] = 0.05
                lowres[py:py + ph, px:px + pw] = 0.9
                taken[py - 2:py + ph + 2, px - 2:px + pw + 2] = True
                break
        else:
            raise RuntimeError("no room")
    H, W = 4 * h - 2, 4 * w - 1
    cam = F.interpolate(torch.from_numpy(lowres)[None, None], (H, W), mode="bilinear", align_corners=True)[0, 0].numpy()
    return cam.astype(np.float32), edge, dp, np.asarray([H, W])


def run_reference(mods, cam, edge, dp, size):
    """the reference's functions in the order its worker calls them; the tensor glue between them is this project's own"""
    indexing, _, L = mods
    H, W = int(size[0]), int(size[1])
    centroids = L.find_centroids_with_refinement(dp)
    instance_map = L.cluster_centroids(centroids, dp)                       # one-hot bool [K,h,w]
    K, h, w = instance_map.shape
    low = F.interpolate(torch.from_numpy(cam).reshape(1, 1, *cam.shape), size=(h, w), mode="bilinear", align_corners=True)[0]
    instance_cam = L.separte_score_by_mask(low, instance_map)               # [1,K,h,w]
    rw = indexing.propagate_to_edge(instance_cam, torch.from_numpy(edge), radius=5, beta=BETA, exp_times=EXP_TIMES)   # [K,1,h,w]
    up = F.interpolate(rw, scale_factor=4, mode="bilinear", align_corners=False)[:, 0, :H, :W]
    up = up / up.max()
    stack = torch.cat([torch.full_like(up[:1], BG_THRES), up])             # the background plane first: it wins ties
    labels = stack.argmax(0).numpy()
    planes = labels[None] == np.arange(1, K + 1)[:, None, None]
    det = L.detect_instance(up.numpy(), planes, np.zeros(K, np.int64), max_fragment_size=H * W * 0.01)
    ordered = stack.sort(0).values
    return dict(centroids=centroids, instance_map=instance_map, instance_cam=instance_cam[0].numpy(), rw=rw[:, 0].numpy(),
                rw_up=up.numpy(), labels=labels, det=det, gap=(ordered[-1] - ordered[-2]).numpy())


def main():
    mods = reference_modules()
    for seed in range(100):
        rng = np.random.default_rng(seed)
        try:
            scenes = [make_scene(h, w, nb, rng) for h, w, nb in SCENES]
        except RuntimeError as e:
            print(f"seed {seed}: {e}")
            continue
        outs = [run_reference(mods, *s) for s in scenes]
        n3 = sum(o["instance_map"].shape[0] >= 3 for o in outs)
        small = sum(bool((np.asarray(o["det"]["score"]) == 0).any()) for o in outs)
        tight = max(float((o["gap"] < 1e-3).mean()) for o in outs)
        print(f"seed {seed}: instances {[o['instance_map'].shape[0] for o in outs]}, fragments "
              f"{[len(o['det']['score']) for o in outs]}, scenes with a sub-1% fragment {small}, largest tight share {tight:.5f}")
        split = sum(len(o["det"]["score"]) > o["instance_map"].shape[0] for o in outs)
        if n3 >= 2 and small >= 1 and tight <= 0.005 and split >= 1:
            break
    else:
        raise SystemExit("no seed met the conditions")
    rec = {"beta": np.int32(BETA), "exp_times": np.int32(EXP_TIMES), "bg_thres": np.float32(BG_THRES), "n_scenes": np.int32(len(scenes)),
           "seed": np.int32(seed)}
    pi = mods[0].PathIndex(radius=5, default_size=(23, 36))
    paths = [p for group in pi.search_paths for p in group]           # each [length, 2], the destination first
    rec["path_len"] = np.asarray([len(p) for p in paths], np.int8)
    rec["path_cells"] = np.concatenate(paths).astype(np.int8)
    for i, ((cam, edge, dp, size), o) in enumerate(zip(scenes, outs)):
        assert o["centroids"].dtype == np.int32 and o["instance_map"].dtype == bool
        rec.update({f"s{i}_cam": cam, f"s{i}_edge": edge, f"s{i}_dp": dp, f"s{i}_size": size.astype(np.int32),
                    f"s{i}_centroids": o["centroids"].astype(np.int8),
                    f"s{i}_instance_map": np.argmax(o["instance_map"], 0).astype(np.int8),
                    f"s{i}_instance_cam": o["instance_cam"].astype(np.float32), f"s{i}_rw": o["rw"].astype(np.float32),
                    f"s{i}_rw_up": o["rw_up"].astype(np.float32), f"s{i}_labels": o["labels"].astype(np.int8),
                    f"s{i}_det_score": np.asarray(o["det"]["score"]), f"s{i}_det_class": np.asarray(o["det"]["class"]),
                    f"s{i}_det_mask_bits": np.packbits(o["det"]["mask"]),
                    f"s{i}_det_mask_shape": np.asarray(o["det"]["mask"].shape, np.int32)})
        assert o["det"]["mask"].dtype == bool and o["rw"].dtype == np.float32 and o["rw_up"].dtype == np.float32
        assert (o["instance_map"].sum(0) == 1).all()
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
