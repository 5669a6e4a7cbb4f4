"""Records tests/golden/g19_crf.npz from pydensecrf itself, where it can be imported: the pin of tests/oracle_crf.py against the
library IRNet/misc/imutils.py:169-183 calls.  That pin is OPEN: pydensecrf is installed on no machine this stack is built or tested
on, so this tool has not been run and no fixture is committed.  Until it is, the oracle is a restatement of the published
algorithm, anchored to the exact O(N^2) mean field (tests/test_crf_host.py).

    python tools/gen_golden_crf.py          # needs `import pydensecrf`; never installs anything

Per scene s of tests/oracle_crf.scenes(): `{s}.img`, `{s}.cam`, `{s}.q` float32 [2 CRFs (fg, bg threshold), 2 labels, H, W] =
DenseCRF2D.inference(10) as cam_to_ir_label.py:58-69 sets it up, `{s}.conf` uint8 [H,W] after cam_to_ir_label.py:72-74; plus
`version`, the library's.  tests/test_crf_host.py::test_oracle_equals_a_pydensecrf_recording reads the file when it exists.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "g19_crf.npz")


def inference(dcrf, unary_from_labels, img, labels, t=10, n_labels=2, gt_prob=0.7):
    """imutils.crf_inference_label up to Q"""
    h, w = img.shape[:2]
    d = dcrf.DenseCRF2D(w, h, n_labels)
    d.setUnaryEnergy(unary_from_labels(labels, n_labels, gt_prob=gt_prob, zero_unsure=False))
    d.addPairwiseGaussian(sxy=3, compat=3)
    d.addPairwiseBilateral(sxy=50, srgb=5, rgbim=np.ascontiguousarray(np.copy(img)), compat=10)
    return np.array(d.inference(t), np.float32).reshape(n_labels, h, w)


def main():
    try:
        import pydensecrf
        import pydensecrf.densecrf as dcrf
        from pydensecrf.utils import unary_from_labels
    except ImportError as e:
        raise SystemExit(f"pydensecrf cannot be imported here ({e}): nothing recorded; the pin stays open")
    import oracle_crf as O
    out = {"version": np.array(str(getattr(pydensecrf, "__version__", "unknown")))}
    for name, (img, cam) in O.scenes().items():
        qs = [inference(dcrf, unary_from_labels, img, O.initial_labels(cam, thr)) for thr in (0.3, 0.1)]
        q = np.stack(qs)
        out[f"{name}.img"], out[f"{name}.cam"], out[f"{name}.q"] = img, cam, q
        out[f"{name}.conf"] = O.combine(np.argmax(qs[0], 0), np.argmax(qs[1], 0))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes) from pydensecrf {out['version']}")


if __name__ == "__main__":
    main()
