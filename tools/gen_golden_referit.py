"""Records tests/golden/g19_referit.npz from the REAL reference code, on the CPU: the items of its ReferIt datasets
(dataset/Dataset_referit.py ImageLoader and ImageLoader_train) on the synthetic tree of tests/oracle_referit.py at --size 64.
Build-machine tool: the reference tree is not on the GPU machines, and nothing that runs there reads it.

    python tools/gen_golden_referit.py

The reference is imported through oracle.ref_shim.install_dataset().  torchvision is absent, so the stubbed
`torchvision.transforms` gets working Compose / Resize / ToTensor / Normalize here with torchvision's documented behaviour on PIL
input (Resize((h, w)) = Image.resize((w, h), BILINEAR); ToTensor = uint8 HWC -> float32 CHW / 255; Normalize = (x - mean) / std).
pycocotools is absent too: the shim serves `pycocotools.mask` from tris_amd.dataset.cocomask, so the recorded MASKS are pinned to
cocomask (a restatement of pycocotools' published algorithm), not to pycocotools itself -- cocomask's header says the same.

Recorded: the file order; per test item the surviving keys, word_id, bbox, mask, the image tensor and image_sizes; per train item
the image tensor and word_id.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "g19_referit.npz")
SIZE = 64
MAX_TOKENS = 20


def reference_module():
    from oracle import ref_shim
    ref_shim.install_dataset()
    tvt = sys.modules["torchvision.transforms"]
    tvf = sys.modules["torchvision.transforms.functional"]

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, img):
            for t in self.transforms:
                img = t(img)
            return img

    class Resize:
        def __init__(self, size, interpolation=2):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            return tvf.resize(img, self.size, self.interpolation)

    class ToTensor:
        def __call__(self, pic):
            return tvf.to_tensor(pic)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, t):
            return tvf.normalize(t, self.mean, self.std)

    tvt.Compose, tvt.Resize, tvt.ToTensor, tvt.Normalize = Compose, Resize, ToTensor, Normalize
    import dataset.Dataset_referit as R                       # noqa: E402  (the reference's)
    return R


def main():
    import oracle_referit as O
    from types import SimpleNamespace
    R = reference_module()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = O.synthetic_root(tmp)
        args = SimpleNamespace(size=SIZE, refer_data_root=root, max_query_len=MAX_TOKENS, negative_samples=0)
        ds_train, ds_test = R.get_refit_dataset(args)
        out["files"] = np.array([str(f) for f in ds_test.files])
        for n in range(len(ds_test)):
            img, items, sizes, path = ds_test[n]
            out[f"t{n}_img"] = img.numpy()
            out[f"t{n}_size"] = np.array(sizes, np.int64)
            out[f"t{n}_keys"] = np.array(list(items.keys()), dtype="U8")
            for k, it in items.items():
                out[f"t{n}_{k}_word_id"] = it["word_id"].numpy()
                out[f"t{n}_{k}_bbox"] = np.asarray(it["bbox"])
                out[f"t{n}_{k}_mask"] = it["mask"]
        out["n_train"] = np.array(len(ds_train))
        for n in range(len(ds_train)):
            img, word_id, neg = ds_train[n]
            assert neg == -1
            out[f"r{n}_img"] = img.numpy()
            out[f"r{n}_word_id"] = np.asarray(word_id)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in out.items() if k.endswith("_keys")})


if __name__ == "__main__":
    main()
