"""Records what cv2 gives for the demo's presentation pass, where cv2 can be imported (it is installed on no machine of this
project, so nothing from this script is committed yet):

    python tools/gen_golden_overlay.py [--out tests/golden/overlay_cv2.npz]

The .npz holds
  * `colormap_jet`  uint8 [256,3] RGB: cv2.applyColorMap(arange(256), cv2.COLORMAP_JET), channels turned from BGR to RGB;
  * `heatmap`, `original`, `figure`: one input of the reference's visualize_cam (demo.py:28-39), restated here with an RGB
    picture, and the uint8 [H,W,3] RGB array it returns;
  * `project_jet`   the project's integer table (tris_amd.predict.JET) and `max_abs_difference` between the two tables.

With the file present, a test can pin tris_amd.demo.visualize_cam(heatmap, original, colormap=colormap_jet) == figure, and the
statement "the project's table has not been compared with cv2.COLORMAP_JET" in DESIGN.md / README.md can be replaced by the number.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "overlay_cv2.npz"))
    args = ap.parse_args()
    try:
        import cv2
    except ImportError:
        raise SystemExit("gen_golden_overlay: cv2 cannot be imported here; run this where it is installed")
    from tris_amd.predict import JET
    table = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(256, 1), cv2.COLORMAP_JET)[:, 0, ::-1].copy()
    rng = np.random.RandomState(0)
    heatmap = rng.uniform(0, 1, (37, 50)).astype(np.float32)
    original = rng.randint(0, 256, (37, 50, 3)).astype(np.uint8)
    # visualize_cam (demo.py:28-38) on an RGB picture
    bgr = cv2.applyColorMap(np.uint8(heatmap * 255), cv2.COLORMAP_JET)
    fig = cv2.cvtColor(cv2.addWeighted(bgr, .6, cv2.cvtColor(original, cv2.COLOR_RGB2BGR), 0.4, 0), cv2.COLOR_BGR2RGB)
    diff = int(np.abs(table.astype(int) - JET.astype(int)).max())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, colormap_jet=table, heatmap=heatmap, original=original, figure=fig, project_jet=JET,
                        max_abs_difference=np.int64(diff))
    print(f"wrote {args.out}: cv2.COLORMAP_JET vs the project's table: max |difference| = {diff}")


if __name__ == "__main__":
    main()
