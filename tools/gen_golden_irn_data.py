"""Records tests/golden/g18_irn_data.npz from the REAL reference code, on the CPU: items of IRNet's training dataset.  Build-machine
tool: the reference tree is not on the GPU machines, and nothing that runs there reads it.

    python tools/gen_golden_irn_data.py

What runs is the reference's voc12.dataloader.ReferAffinityDataset.__getitem__ (hor_flip, random crop, rescale (0.5, 1.5), the
indices of misc.indexing.PathIndex(radius=5, default_size=(crop // 4, crop // 4)), as step_refer/train_irn.py:13-26 constructs
it) and ReferImageDataset.__getitem__ with crop_method="top_left" and crop_size (train_irn.py:86-89), with the stubs of
tools/gen_golden_irn_loss.reference_modules; `imageio.imread` is a Pillow decode.  Every call runs under random.seed(k); the
numbers the item draws are recorded from the reference's own calls of the random module.

The images and labels are those of tests/oracle_irn_data.py (synthetic, seeded), written losslessly under the names the lookup
rule wants; the decoded arrays are stored in the fixture.  Recorded per case: img, label, the three affinity label arrays, the
draw.  The fixture also records how many cases took each branch; every branch must occur or the run fails (choose other seeds).
"""
import json
import os
import random
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "g18_irn_data.npz")
CROP = 40
RADIUS = 5
N_CASES = 24
NAMES = ["g18_0_1", "g18_1_2", "g18_2_2", "g18_3_3", "g18_4_4", "g18_5_5"]      # image 2 serves two expressions; image 5 is grey


def image_index(name):
    return int(name.split("_")[-1]) - 1


def write_inputs(root, labels):
    import oracle_irn_data as O
    os.makedirs(labels)
    for name in NAMES:
        i = image_index(name)
        Image.fromarray(O.synthetic_image(i)).save(os.path.join(root, f"COCO_train2014_{str(i + 1).zfill(12)}.jpg"), format="PNG")
        Image.fromarray(O.synthetic_label(i)).save(os.path.join(labels, name + ".png"))
    with open(os.path.join(root, "names.json"), "w") as f:
        json.dump(NAMES, f)
    return os.path.join(root, "names.json")


class Recorder:
    """the numbers an item draws, from the reference's own calls of the random module, in order"""

    def __enter__(self):
        self.calls, self.saved = [], {k: getattr(random, k) for k in ("random", "getrandbits", "randrange")}
        for k, fn in self.saved.items():
            setattr(random, k, self.wrap(k, fn))
        return self

    def wrap(self, k, fn):
        def f(*a):
            v = fn(*a)
            self.calls.append((k, v))
            return v
        return f

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(random, k, fn)


def main():
    import oracle_irn_data as O
    from gen_golden_irn_loss import reference_modules
    _, PathIndex, _ = reference_modules()
    sys.modules["imageio"].imread = lambda path: np.asarray(Image.open(path))
    import voc12.dataloader as dataloader          # noqa: E402  (the reference's)
    rec = {"crop": np.int32(CROP), "radius": np.int32(RADIUS)}
    branches = {k: 0 for k in ("pad_x", "crop_x", "pad_y", "crop_y", "flip", "no_flip", "axis_unchanged", "offset_zero",
                               "offset_max")}
    with tempfile.TemporaryDirectory() as tmp:
        root, labels = os.path.join(tmp, "train2014"), os.path.join(tmp, "ir_label")
        os.makedirs(root)
        names = write_inputs(root, labels)
        pi = PathIndex(radius=RADIUS, default_size=(CROP // 4, CROP // 4))
        ds = dataloader.ReferAffinityDataset(img_name_list_path=names, label_dir=labels, voc12_root=root,
                                             indices_from=pi.src_indices, indices_to=pi.dst_indices, hor_flip=True,
                                             crop_size=CROP, crop_method="random", rescale=(0.5, 1.5))
        infer = dataloader.ReferImageDataset(img_name_list_path=names, crop_size=CROP, data_root=root, crop_method="top_left")
        for i in sorted({image_index(n) for n in NAMES}):
            rec[f"image{i}"] = O.synthetic_image(i)
        for j, name in enumerate(NAMES):
            rec[f"label{j}"] = O.synthetic_label(image_index(name))
        seeds = []
        k = 0
        while len(seeds) < N_CASES:
            idx = len(seeds) % len(NAMES)
            random.seed(k)
            with Recorder() as r:
                out = ds[idx]
            kinds = [c[0] for c in r.calls]
            assert kinds == ["random", "getrandbits", "randrange", "randrange"], kinds
            u, bit, rx, ry = (c[1] for c in r.calls)
            H, W = rec[f"image{image_index(NAMES[idx])}"].shape[:2]
            scale = 0.5 + u * 1.0
            h, w = int(np.round(H * scale)), int(np.round(W * scale))
            tags = ["crop_x" if w > CROP else "pad_x", "crop_y" if h > CROP else "pad_y", "flip" if bit else "no_flip"]
            if (h == H) != (w == W):
                tags.append("axis_unchanged")
            for off, n in ((rx, w), (ry, h)):
                if n != CROP:
                    tags += ["offset_zero"] if off == 0 else (["offset_max"] if off == abs(n - CROP) else [])
            # until every branch has been taken twice, keep only the seeds that add to one still short of that
            k += 1
            if not any(branches[t] < 2 for t in tags) and any(v < 2 for v in branches.values()):
                continue
            n = len(seeds)
            seeds.append(k - 1)
            for t in tags:
                branches[t] += 1
            rec[f"c{n}_index"] = np.int32(idx)
            rec[f"c{n}_seed"] = np.int32(k - 1)
            rec[f"c{n}_draw"] = np.asarray([u, bit, rx, ry], np.float64)
            rec[f"c{n}_img"] = np.ascontiguousarray(out["img"])                       # float32 [3, crop, crop]
            rec[f"c{n}_label"] = np.ascontiguousarray(out["label"])
            for key in ("aff_bg_pos_label", "aff_fg_pos_label", "aff_neg_label"):
                rec[f"c{n}_{key}"] = (out[key].numpy() != 0)                          # 0 / 1 values: stored as bool
                assert np.array_equal(rec[f"c{n}_{key}"].astype(np.float32), out[key].numpy())
            assert rec[f"c{n}_img"].dtype == np.float32 and rec[f"c{n}_label"].dtype == np.uint8
        for j in range(len(NAMES)):
            random.seed(j)
            with Recorder() as r:
                out = infer[j]
            assert not r.calls, r.calls                                               # the top-left mode draws nothing
            rec[f"t{j}_img"] = np.ascontiguousarray(out["img"])
    print("seeds", seeds)
    print("branches", branches)
    missing = [k for k, v in branches.items() if v == 0]
    assert not missing, f"branches that no case took: {missing}"
    rec["branch_names"] = np.asarray(list(branches))
    rec["branch_counts"] = np.asarray(list(branches.values()), np.int32)
    rec["n_cases"] = np.int32(N_CASES)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 900_000


if __name__ == "__main__":
    main()
