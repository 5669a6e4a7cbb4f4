"""IRNet's dense-CRF label pass on the MI355X (csrc/crf.hip, tris_amd.crf, tris_amd.cam_to_ir_label) against tests/oracle_crf.py.

Geometry (keys, barycentric weights, the vertex set, the neighbour table) is compared for equal bits.  Values are compared with
the fp64 oracle; the bound is 8 x the distance of the oracle's own fp32 run from its fp64 run on the same input (the convention
of tests/test_gpu_stage2.py), with a floor of 4 fp32 eps.  The oracle restates the published algorithm and is anchored to the
exact mean field by tests/test_crf_host.py; it has not been compared with a recording of pydensecrf."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import oracle_crf as O
from conftest import ROOT

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
FLOOR = 4 * EPS
SCENES = list(O.scenes())


@pytest.fixture(scope="module")
def scenes():
    return O.scenes()


@pytest.fixture(scope="module")
def oracle(scenes):
    """per scene the oracle's lattices in both value arithmetics (the geometry is float32 in both), computed once"""
    return {name: (O.Lattices(img, np.float64), O.Lattices(img, np.float32)) for name, (img, _) in scenes.items()}


@pytest.fixture(scope="module")
def device(scenes):
    from tris_amd import crf
    return {name: crf.DenseCrfLattices(img) for name, (img, _) in scenes.items()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("d", [2, 5])
def test_lattice_points_equal_the_oracle_bit_for_bit(scenes, oracle, device, d):
    for name in SCENES:
        want = oracle[name][0].gauss if d == 2 else oracle[name][0].bilat
        got = device[name].gauss if d == 2 else device[name].bilat
        keys, bary = got.keys.cpu().numpy(), got.bary.cpu().numpy()
        assert keys.shape == want.packed.shape and (keys == want.packed).all(), name          # per pixel, the d+1 keys in order r
        assert (_bits(bary) == _bits(want.bary)).all(), (name, np.abs(bary - want.bary).max())
        uniq = got.uniq.cpu().numpy()
        assert got.M == want.M and (uniq == want.uniq).all(), (name, got.M, want.M)
        assert (got.inv.cpu().numpy() == want.inv).all(), name


@pytest.mark.parametrize("d", [2, 5])
def test_neighbour_table_and_vertex_lists_equal_the_oracle(oracle, device, d):
    for name in SCENES:
        want = oracle[name][0].gauss if d == 2 else oracle[name][0].bilat
        got = device[name].gauss if d == 2 else device[name].bilat
        nbr = got.nbr.cpu().numpy()
        assert nbr.shape == (d + 1, 2, want.M) and nbr.dtype == np.int32
        assert (nbr == want.nbr).all(), (name, int((nbr != want.nbr).sum()))                 # both in sorted-key order, -1 included
        assert (nbr == -1).any(), name
        # the per-vertex lists: every (pixel, r) once, grouped by vertex, ascending within a vertex
        order, off = got.order.cpu().numpy().astype(np.int64), got.off.cpu().numpy()
        inv = want.inv.ravel()
        assert off[0] == 0 and off[-1] == inv.size and (np.sort(order) == np.arange(inv.size)).all(), name
        assert (np.diff(inv[order]) >= 0).all() and (off[1:] == np.cumsum(np.bincount(inv, minlength=want.M))).all(), name
        same = np.diff(inv[order]) == 0
        assert (np.diff(order)[same] > 0).all(), name


# ------------------------------------------------------------------------------------------------------------ one filter pass
@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("C", [1, 4])
def test_filter_pass_against_the_fp64_oracle(oracle, device, C, normalised):
    rng = np.random.default_rng(100 + C)
    for name in ("s48x64", "s1x40", "grey33x40", "s1x1"):
        for which in ("gauss", "bilat"):
            L64, L32, got = (getattr(x, which) for x in (*oracle[name], device[name]))
            n64 = getattr(oracle[name][0], "norm_" + which[0]) if normalised else None
            n32 = getattr(oracle[name][1], "norm_" + which[0]) if normalised else None
            x = rng.random((L64.N, C)).astype(np.float32)
            want = O.filter(L64, x, n64, np.float64)
            own = _rel(O.filter(L32, x, n32, np.float32), want)
            bound = max(8 * own, FLOOR)
            xd = torch.from_numpy(x).cuda()
            out = got.filter(xd, normalised=normalised)
            err = _rel(out.cpu().numpy(), want)
            print(f"{name} {which} C={C} norm={normalised}: kernel {err:.3e}, oracle fp32 {own:.3e}, bound {bound:.3e}")
            assert err <= bound, (name, which, err, bound)
            again = got.filter(xd, normalised=normalised)
            assert torch.equal(out.view(torch.int32), again.view(torch.int32)), (name, which)
            if normalised:
                assert _rel(got.norm.cpu().numpy(), n64) <= max(8 * _rel(n32, n64), FLOOR), (name, which)


# --------------------------------------------------------------------------------------------------------------- the full pass
@pytest.mark.parametrize("name", SCENES)
def test_ir_label_against_the_fp64_oracle(scenes, oracle, device, name):
    from tris_amd import crf
    img, cam = scenes[name]
    lat64, lat32 = oracle[name]
    want, q64 = O.ir_label(img, cam, lattices=lat64, return_q=True)
    _, q32 = O.ir_label(img, cam, lattices=lat32, value_dtype=np.float32, return_q=True)
    own = _rel(q32, q64)
    bound = max(8 * own, FLOOR)
    conf, q = crf.ir_label(cam, device[name], return_q=True)
    assert conf.dtype == torch.uint8 and tuple(conf.shape) == cam.shape and tuple(q.shape) == (2, 2) + cam.shape
    err = _rel(q.cpu().numpy(), q64)
    print(f"{name}: Q kernel {err:.3e}, oracle fp32 {own:.3e}, bound {bound:.3e}")
    assert err <= bound, (name, err, bound)
    sure = (np.abs(q64[:, 1] - q64[:, 0]) > bound * np.abs(q64).max()).all(0)       # the oracle margin of both CRFs
    left_out = 1.0 - sure.mean()
    assert left_out <= 0.01, (name, left_out)
    got = conf.cpu().numpy()
    assert (got[sure] == want[sure]).all(), (name, int((got[sure] != want[sure]).sum()))
    if name in ("s48x64", "s96x128"):
        assert set(np.unique(got)) == {0, 1, 255}, name
    # launched twice: equal bytes
    conf2, q2 = crf.ir_label(cam, device[name], return_q=True)
    assert torch.equal(conf, conf2) and torch.equal(q.view(torch.int32), q2.view(torch.int32))


def test_strict_threshold_and_negative_values_on_the_device(scenes):
    from tris_amd import ops
    _, cam = scenes["ties31x37"]
    U, Q = ops.crf_unary_cam(torch.from_numpy(cam).cuda(), 0.3, 0.1, *(float(np.float32(-np.log(p))) for p in (0.7, 0.3)))
    U = U.cpu().numpy().reshape(-1, 2, 2)
    for r, thr in enumerate((0.3, 0.1)):
        want = O.unary_from_labels(O.initial_labels(cam, thr))                     # [2, N]
        assert (_bits(U[:, r, :].T) == _bits(want)).all(), thr
    q = O.softmax_neg(-U.astype(np.float64).transpose(2, 0, 1))
    assert np.abs(Q.cpu().numpy().reshape(-1, 2, 2).transpose(2, 0, 1) - q).max() <= 4 * EPS


def test_lattices_are_shared_between_the_names_of_an_image(scenes, device):
    from tris_amd import crf
    img, cam = scenes["s48x64"]
    other = np.ascontiguousarray(cam[::-1] * np.float32(0.8))
    shared = [crf.ir_label(c, device["s48x64"], return_q=True) for c in (cam, other)]
    fresh = [crf.ir_label(c, crf.DenseCrfLattices(img), return_q=True) for c in (cam, other)]
    for (c0, q0), (c1, q1) in zip(shared, fresh):
        assert torch.equal(c0, c1) and torch.equal(q0.view(torch.int32), q1.view(torch.int32))
    assert not torch.equal(shared[0][0], shared[1][0])


def test_crf_inference_label_equals_the_path_through_ir_label(scenes, device):
    from tris_amd import crf
    img, cam = scenes["grey33x40"]
    _, q = crf.ir_label(cam, device["grey33x40"], return_q=True)
    for r, thr in enumerate((0.3, 0.1)):
        labels = O.initial_labels(cam, thr)
        pred = crf.crf_inference_label(img, labels, lattices=device["grey33x40"] if r else None)
        assert pred.dtype == torch.int64 and torch.equal(pred, (q[r, 1] > q[r, 0]).to(torch.int64)), thr
    with pytest.raises(ValueError, match="does not go with"):
        crf.ir_label(cam[:-1], device["grey33x40"])


# ------------------------------------------------------------------------------------------------------------------ the command
def test_command_line_writes_the_labels_train_irn_reads(scenes, device, tmp_path):
    from tris_amd import crf
    from tris_amd.dataset.irn_data import HbmIrnCache, ReferAffinityData
    a, b = scenes["s48x64"], scenes["grey33x40"]
    names = ["x_0_11", "x_1_11", "y_0_12"]                                   # three names over two images
    cams = [a[1], np.ascontiguousarray(a[1][::-1] * np.float32(0.8)), b[1]]
    lats = [device["s48x64"], device["s48x64"], device["grey33x40"]]
    root, D, L = tmp_path / "train2014", tmp_path / "cam", tmp_path / "ir_label"
    root.mkdir()
    D.mkdir()
    for i, img in ((11, a[0]), (12, b[0])):
        Image.fromarray(img).save(root / f"COCO_train2014_{str(i).zfill(12)}.jpg", format="PNG")     # lossless, under the rule's name
    for name, cam in zip(names, cams):
        np.save(D / f"{name}.npy", cam)
    (tmp_path / "names.json").write_text(json.dumps(names))
    cmd = [sys.executable, "-m", "tris_amd.cam_to_ir_label", "--cam_out_dir", str(D), "--voc12_root", str(root), "--train_list",
           str(tmp_path / "names.json"), "--ir_label_out_dir", str(L), "--num_workers", "4"]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)      # a fresh process with its own limit
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "dense-CRF lattices: 2 builds for 3 names" in run.stdout, run.stdout
    for name, cam, lat in zip(names, cams, lats):
        with Image.open(L / f"{name}.png") as im:
            assert im.mode == "L" and im.size == (cam.shape[1], cam.shape[0]), name
            got = np.asarray(im)
        assert (got == crf.ir_label(cam, lat).cpu().numpy()).all(), name
    # what train_irn does with the directory before its first step (its ReferAffinityData and HbmIrnCache, through the label
    # reader of tris_amd.dataset.irn_data); the command itself would need a ResNet-50 file no test can make in a second
    data = ReferAffinityData(str(tmp_path / "names.json"), str(L), str(root), crop_size=128)
    cache = HbmIrnCache(data, "cuda")
    assert len(cache) == 3 and len(cache.image_offsets) == 2
    assert (data.load_label(2, size=b[1].shape) == crf.ir_label(cams[2], lats[2]).cpu().numpy()).all()
    # a map of another size: non-zero exit, the file is named
    np.save(D / "y_0_12.npy", b[1][:-1])
    bad = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "y_0_12.npy" in bad.stderr and "does not go with" in bad.stderr, bad.stderr[-2000:]
