"""The box-metric restatement (tests/oracle_boxes.py) against hand-derived cases -- no GPU.  generate_bbox needs cv2, which
is on no machine of this project, so no golden can be recorded: these cases are what anchors the oracle that the device pass
(csrc/boxes.hip) is compared with in tests/test_gpu_boxes.py."""
import os

import numpy as np
import pytest

import oracle_boxes as OB
from conftest import ROOT


def block7x9():
    m = np.zeros((7, 9), bool)
    m[1:6, 1:6] = True
    m[3, 3] = False
    m[0, 8] = m[6, 7] = True
    return m


def ring9():
    m = np.zeros((9, 9), bool)
    m[1:8, 1:8] = True
    m[2:7, 2:7] = False
    m[4, 4] = True
    return m


def frame5x6():
    m = np.ones((5, 6), bool)
    m[1:4, 1:5] = False
    return m


def checker8():
    i, j = np.indices((8, 8))
    return (i + j) % 2 == 0


def dots(n):
    m = np.zeros((n, n), bool)
    m[::2, ::2] = True
    return m


def row7():
    return np.array([[1, 0, 1, 1, 0, 0, 1]], bool)


def test_block_with_hole_and_specks():
    m = block7x9()
    assert OB.proposals(m) == [(8, 0, 1, 1), (1, 1, 5, 5), (2, 2, 3, 3), (7, 6, 1, 1)]
    assert OB.generate_bbox(m) == [(8, 0, 9, 1, 1.0), (7, 6, 8, 7, 1.0), (1, 1, 6, 6, 0.9600000000000001)]
    # the hole's box (2,2,3,3) against the block's (1,1,5,5), both read as x1y1x2y2: inter 1, areas 16 and 1
    keep = OB.nms([(1, 1, 5, 5), (2, 2, 3, 3)], [0.96, 8 / 9])
    assert keep == [0]
    assert np.float32(1) / np.float32(16) == np.float32(0.0625) and 0.0625 > 0.05


def test_ring_with_dot():
    m = ring9()
    assert OB.proposals(m) == [(1, 1, 7, 7), (1, 1, 7, 7), (4, 4, 1, 1)]
    assert OB.generate_bbox(m) == [(4, 4, 5, 5, 1.0), (1, 1, 8, 8, 25 / 49)]


def test_all_ones_frame():
    m = frame5x6()
    assert OB.proposals(m) == [(0, 0, 6, 5), (0, 0, 6, 5)]
    out = OB.generate_bbox(m)
    assert len(out) == 1 and out[0][:4] == (0, 0, 6, 5) and out[0][4] == 0.6


def test_checkerboard():
    m = checker8()
    props = OB.proposals(m)
    assert len(props) == 19 and props.count((0, 0, 8, 8)) == 1
    assert sum(1 for p in props if p[2:] == (3, 3)) == 18
    out, info = OB.generate_bbox(m, full=True)
    assert len(out) == 16
    assert out[:3] == [(0, 0, 8, 8, 0.5), (3, 0, 6, 3, 4 / 9), (5, 0, 8, 3, 4 / 9)]
    assert (1, 0, 3, 3) in props and (1, 0, 4, 3) not in [b[:4] for b in out]     # the hole at (1,2): ovr = 6/64 > 0.05
    assert (3, 0, 3, 3) in props                                                  # zero width as xyxy: never suppressed
    assert OB.nms([(0, 0, 8, 8), (1, 0, 3, 3)], [0.5, 4 / 9]) == [0]
    assert OB.nms([(0, 0, 8, 8), (3, 0, 3, 3)], [0.5, 4 / 9]) == [0, 1]


def test_dots_tie_rule_is_raster_order():
    m = dots(16)
    props = OB.proposals(m)
    assert len(props) == 64 and all(p[2:] == (1, 1) for p in props)
    out = OB.generate_bbox(m)
    assert [b[:2] for b in out] == [(x, y) for y in range(0, 16, 2) for x in range(0, 16, 2)]
    assert all(b[4] == 1.0 for b in out)


def test_one_pixel_and_row():
    for v in (0, 1):
        assert OB.generate_bbox(np.full((1, 1), v, bool)) == OB.DEFAULT
    assert OB.generate_bbox(np.zeros((5, 7), bool)) == OB.DEFAULT and OB.generate_bbox(np.ones((5, 7), bool)) == OB.DEFAULT
    m = row7()
    assert OB.proposals(m) == [(0, 0, 1, 1), (2, 0, 2, 1), (6, 0, 1, 1)]
    assert len(OB.generate_bbox(m)) == 3


def test_confidence_is_numpys_last_bit():
    m = block7x9()
    assert OB.confidences(m, [(1, 1, 5, 5)])[0] == 0.9600000000000001 != 24 / 25


def test_bbox_hit_last_match_wins_and_first_box_fallback():
    m = ring9()                                                # kept: (4,4,5,5) then (1,1,8,8)
    tgt = np.zeros((9, 9), bool)
    tgt[4, 4] = True
    r = OB.sentence(m, tgt, [1, 1, 8, 8], (4, 4))              # the arg-max lies in both: the LAST one is taken
    assert r["bbox_hit"] == (1, 1, 8, 8) and r["hitm"] == 1 and r["box_miou"] == np.float32(1) and r["box_acc"] == 1
    r = OB.sentence(m, tgt, [1, 1, 8, 8], (0, 0))              # in none: the first kept box
    assert r["bbox_hit"] == (4, 4, 5, 5) and r["hitm"] == 0
    assert r["box_miou"] == np.float32(1) / np.float32(49) and r["box_acc"] == 1
    r = OB.sentence(m, tgt, [0, 0, 2, 2], (5, 5))              # both ends inclusive: (5,5) is the dot box's corner too
    assert r["bbox_hit"] == (1, 1, 8, 8)
    assert r["box_miou"] == np.float32(1) / np.float32(52) and r["box_acc"] == 0
    assert (r["n_prop"], r["n_nms"], r["n_kept"]) == (3, 2, 2) and r["cmax"] == 1.0


def test_default_list_metrics():
    z = np.zeros((4, 6), bool)
    r = OB.sentence(z, np.ones((4, 6), bool), [0, 0, 1, 1], (2, 3))
    assert r["bbox_hit"] == (0, 0, 1, 1) and r["box_miou"] == np.float32(1) and r["box_acc"] == 1 and r["hitm"] == 1
    assert (r["n_prop"], r["n_nms"], r["n_kept"]) == (0, 0, 0)
    r = OB.sentence(z, np.ones((4, 6), bool), [0, 0, 2, 2], (0, 0))
    assert r["box_miou"] == np.float32(0.25) and r["box_acc"] == 0


def test_meters_follow_the_reference_types():
    mt = OB.Meters()
    for v, a, h in ((np.float32(1) / np.float32(3), 1, 1), (np.float32(0.1), 0, 0), (np.float32(0.7), 1, 1)):
        mt.update({"hitm": h, "box_miou": v, "box_acc": a})
    res = mt.result()
    s = np.float32(np.float32(np.float32(1) / np.float32(3) + np.float32(0.1)) + np.float32(0.7))
    assert res["box_miou"] == float(np.float32(100) * (s / np.float32(3)))
    assert res["box_acc"] == float(np.float32(100) * (np.float32(2) / np.float32(3)))
    assert res["hitm"] == 2 / 3 * 100 and res["n_sent"] == 3


def test_colour_map_front_end():
    """utils/box_eval_utils.py:26-47 on a 0/1 input: cubehelix sends {0, 1, NaN} to grey {0, 255, 0}, so the threshold at 127
    keeps the foreground and a 0/0-normalised (degenerate) mask keeps nothing"""
    plt = pytest.importorskip("matplotlib.pyplot")
    cmap = plt.get_cmap("cubehelix")
    with np.errstate(all="ignore"):
        rgb = (cmap(np.array([[0.0, 1.0, np.nan]]))[..., :3].astype("float32") * 255.0).astype("uint8")
    assert rgb.reshape(3, 3).tolist() == [[0, 0, 0], [255, 255, 255], [0, 0, 0]]


def test_header_and_library_carry_the_entry_points():
    import ctypes
    from tris_amd import _lib
    decls, _ = _lib.parse_header()
    assert decls["tris_eval_boxes_workspace_bytes"][0] is ctypes.c_long and len(decls["tris_eval_boxes_workspace_bytes"][1]) == 2
    assert len(decls["tris_eval_boxes_f32"][1]) == 10
    src = open(os.path.join(ROOT, "include", "tris_hip.h")).read()
    head = src[:src.index("long tris_eval_boxes_workspace_bytes")]
    assert "box_eval_utils.py:10-73" in head[-2500:] and "validate.py:106-117" in head[-2500:]
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIBPATH)
    assert hasattr(lib, "tris_eval_boxes_f32") and hasattr(lib, "tris_eval_boxes_workspace_bytes")
    assert _lib.query("tris_eval_boxes_workspace_bytes", 427, 640) > 427 * 640 * 4
    assert _lib.query("tris_eval_boxes_workspace_bytes", 4096, 4097) == -1         # beyond 2^24 pixels
    from tris_amd.config import cfg
    assert cfg.eval_boxes is False or os.environ.get("TRIS_EVAL_BOXES") not in (None, "", "0")
    from tris_amd import validate
    assert validate.last_metrics() is None
