"""The heat-map overlay and the single-image demo without a GPU: the C ABI of csrc/overlay.hip, the colour-table rule, the
integer blend, the restatement (tests/oracle_overlay.py) against a case derived by hand, the near-step cap on every input of
tests/test_gpu_overlay.py, the reference's names in tris_amd.demo and the command's missing-checkpoint error."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_overlay as OV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entries():
    from tris_amd import _lib
    decls, consts = _lib.parse_header()
    assert decls["tris_cam_paint_workspace_bytes"] == (ctypes.c_long, [ctypes.c_int] * 3)
    ret, args = decls["tris_cam_paint_f32"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert ret is ctypes.c_int and args == [P, I, I, I, P, I, I, P, I, P, P, P, P, P, P]
    assert consts["TRIS_PAINT_MINMAX"] == 0 and consts["TRIS_PAINT_UNIT"] == 1
    src = open(os.path.join(ROOT, "include", "tris_hip.h")).read()
    assert "demo.py:28-48, 94-96" in src[src.index("csrc/overlay.hip"):src.index("tris_cam_paint_f32")]
    assert "overlay" in open(os.path.join(ROOT, "tris_amd", "csrc", "build.sh")).read().split("for f in ")[1].split(";")[0].split()
    if not os.path.exists(_lib.LIBPATH):
        pytest.fail(f"{_lib.LIBPATH} is not built")
    lib = ctypes.CDLL(_lib.LIBPATH)
    assert hasattr(lib, "tris_cam_paint_f32") and hasattr(lib, "tris_cam_paint_workspace_bytes")
    # the size query is host code: K sentences of 256 (min, max, arg-max) partials; refuses an empty grid
    q = lib.tris_cam_paint_workspace_bytes
    q.restype = ctypes.c_long
    assert q(0, 4, 4) == 0 and q(3, 480, 640) == 3 * 256 * 16 and q(1, 0, 4) == -1


def test_jet_table_rule():
    from tris_amd.predict import JET, jet_table
    t = OV.jet_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert np.array_equal(t, JET) and np.array_equal(t, jet_table())            # the package's vectorised form, the same table
    assert tuple(t[0]) == (0, 0, 128) and tuple(t[255]) == (128, 0, 0)          # dark blue, dark red
    # the plateaux of the piecewise-linear jet, 64 entries each: blue, then green (cyan to yellow: (0, 255, 255)-type colours
    # where two plateaux meet), then red
    for i, (r, g, b) in enumerate(t.tolist()):
        assert (b == 255) == (32 <= i <= 95) and (g == 255) == (96 <= i <= 159) and (r == 255) == (160 <= i <= 223), i
    assert t[95].tolist() == [0, 253, 255] and t[96].tolist() == [2, 255, 254]   # cyan, where blue's plateau hands over to green's
    assert t[159].tolist() == [254, 255, 2] and t[160].tolist() == [255, 253, 0]  # yellow
    assert (t[:96, 0] == 0).all() and (t[160:, 2] == 0).all() and (t[:32, 1] == 0).all() and (t[224:, 1] == 0).all()
    for ch in range(3):                                                          # every channel rises, then falls
        d = np.sign(np.diff(t[:, ch].astype(int)))
        d = d[d != 0]
        assert (np.diff(d) <= 0).all() and d[0] > 0 and d[-1] < 0, ch


def test_integer_blend_is_round_to_nearest_of_the_weighted_sum():
    c, p = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    exact = 0.6 * c.astype(np.float64) + 0.4 * p.astype(np.float64)
    # (3 c + 2 p) / 5 is a multiple of 1/5: never a half, so every rounding mode of "nearest" agrees
    frac = (3 * c + 2 * p) % 5
    assert not (2 * frac == 5).any()
    want = np.rint(exact).astype(np.int64)
    assert np.abs(want - exact).max() <= 0.4 + 1e-9
    got = OV.blend(c.astype(np.uint8), p.astype(np.uint8))
    assert got.shape == (256, 256) and np.array_equal(got.astype(np.int64), want)


def test_oracle_against_a_case_derived_by_hand():
    """2x2 -> 3x3, align_corners=True: scale 1/2, so the middle row / column sit half-way.
        source  [[-1, 1],      resized [[-1,  0,    1  ],     clamped [[0, 0,    1  ],
                 [ 3, 2]]               [ 1,  1.25, 1.5],              [1, 1.25, 1.5],
                                        [ 3,  2.5,  2  ]]              [3, 2.5,  2  ]]
    lo = 0, hi = 3 at raster index 6; n = u / 3.00001; v = 255 n -> indices below (84.99.. and 254.99.. sit near a step)."""
    m = np.array([[[-1.0, 1.0], [3.0, 2.0]]], np.float32)
    r = OV.paint(m, 3, 3)
    u = np.array([[0, 0, 1], [1, 1.25, 1.5], [3, 2.5, 2]], np.float64)
    assert np.array_equal(r["range"], [[0.0, 3.0]]) and r["argmax"].tolist() == [6]
    den = 3.0 + float(np.float32(1e-5))
    assert np.allclose(r["norm"][0], u / den, rtol=0, atol=1e-15)
    assert r["index"][0].tolist() == [[0, 0, 84], [84, 106, 127], [254, 212, 169]]
    assert r["near"][0].tolist() == [[False, False, True], [True, False, False], [True, False, True]]
    lut = OV.jet_table()
    assert np.array_equal(r["heat"][0, 1, 1], lut[106]) and np.array_equal(r["heat"][0, 0, 0], lut[0])
    img = np.full((3, 3, 3), 200, np.uint8)
    rb = OV.paint(m, 3, 3, img)
    assert rb["heat"][0, 0, 0].tolist() == [(3 * 0 + 400 + 2) // 5, (0 + 400 + 2) // 5, (3 * 128 + 400 + 2) // 5]
    # unit mode: no normalisation, values above 1 saturate
    ru = OV.paint(m, 3, 3, mode=OV.UNIT)
    assert ru["index"][0].tolist() == [[0, 0, 255], [255, 255, 255], [255, 255, 255]] and np.array_equal(ru["range"], [[0.0, 3.0]])
    # a 1-pixel source and a 1-pixel output are legal
    assert OV.paint(np.array([[[0.5]]], np.float32), 2, 3)["index"].tolist() == [[[0, 0, 0], [0, 0, 0]]]
    assert OV.paint(m, 1, 1)["range"].tolist() == [[0.0, 0.0]]


def test_near_step_cap_holds_on_every_gpu_test_input():
    fr = {}
    for Sh, Sw, H, W, K in OV.SHAPES:
        fr[(Sh, Sw, H, W, K)] = OV.near_fraction(OV.paint(OV.case_maps(Sh, Sw, K), H, W))
    for name, (maps, (H, W), mode) in OV.special_cases().items():
        fr[name] = OV.near_fraction(OV.paint(maps, H, W, mode=mode))
    print(fr)
    assert max(fr.values()) <= OV.NEAR_CAP, fr
    # the specials are what they claim to be
    sp = OV.special_cases()
    assert (sp["all_negative"][0] < 0).all() and (sp["signed"][0] < 0).any() and (sp["signed"][0] > 0).any()
    two = OV.paint(sp["two_maxima"][0], 40, 40)
    assert two["argmax"].tolist() == [300] and sp["two_maxima"][0].reshape(-1)[600] == sp["two_maxima"][0].max()
    for name in ("all_negative", "constant"):
        r = OV.paint(sp[name][0], *sp[name][1])
        assert (r["range"][:, 0] == r["range"][:, 1]).all() and not r["index"].any()
    for Sh, Sw, H, W, K in OV.SHAPES[2:]:                                       # a unique maximum: arg-max is decidable
        for m in OV.case_maps(Sh, Sw, K):
            u = np.maximum(OV.upsample(m, H, W), 0)
            assert (u == u.max()).sum() == 1


def test_demo_functions_keep_the_reference_names():
    from tris_amd import demo, dropin
    lead = {"get_transform": ["size"],                                           # demo.py:14
            "visualize_cam": ["normalized_heatmap", "original", "root"],         # demo.py:28
            "get_norm_cam": ["cam"],                                             # demo.py:41
            "prepare_data": ["img_path", "text", "max_length"]}                  # demo.py:50
    for name, want in lead.items():
        params = list(inspect.signature(getattr(demo, name)).parameters.values())
        assert [p.name for p in params[:len(want)]] == want, name
        assert all(p.default is not inspect.Parameter.empty for p in params[len(want):]), name      # appended ones are optional
    sig = inspect.signature(demo.prepare_data).parameters
    assert sig["max_length"].default == 20 and sig["size" if "size" in sig else "img_size"].default == 320
    assert inspect.signature(demo.get_transform).parameters["size"].default is None
    assert "demo" not in dropin.ALIASES                                         # too generic a name for a top-level alias
    from tris_amd.args import get_parser
    a = get_parser().parse_args(["--img", "a.png", "--text", "man, on the right", "--vis_out", "o", "--pretrain", "c.pth"])
    assert (a.img, a.text, a.vis_out) == ("a.png", "man, on the right", "o")


def test_get_transform_is_the_evaluation_transform():
    import torch
    from PIL import Image
    from tris_amd import demo
    from tris_amd.dataset.transform import get_transform
    img = Image.fromarray(OV.case_image(50, 37))
    want, _ = get_transform(64, train=False)(img, Image.new("L", (37, 50)))
    assert torch.equal(demo.get_transform(64)(img), want)
    assert demo.get_transform()(img).shape == (3, 50, 37)


def test_command_names_a_missing_checkpoint(tmp_path):
    missing = tmp_path / "no_such_checkpoint.pth"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tris_amd.demo", "--img", str(tmp_path / "x.png"), "--text", "man on the right",
                        "--pretrain", str(missing), "--size", "64"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "no_such_checkpoint.pth" in r.stderr, (r.returncode, r.stderr[-400:])
    # ... also as a name under --output
    r = subprocess.run([sys.executable, "-m", "tris_amd.demo", "--img", str(tmp_path / "x.png"), "--text", "t", "--output",
                        str(tmp_path), "--pretrain", "no_such_checkpoint.pth"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0 and os.path.join(str(tmp_path), "no_such_checkpoint.pth") in r.stderr


def test_ops_refuse_off_the_device():
    import torch
    from tris_amd import ops
    with pytest.raises(ops.NoGpuError):
        ops.cam_paint(torch.zeros(1, 4, 4))
